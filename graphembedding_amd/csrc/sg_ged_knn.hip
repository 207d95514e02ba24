// sg_ged_knn.hip — the k nearest database graphs of every query under exact graph edit
// distance (include/siamese_ged_knn.h): filter by the bipartite bounds, verify under a cutoff.
// Five launches per call, stream-ordered, no host synchronisation: the m + n entries
// (sg_ged_common.h), the seed bounds of every pair, per row the threshold tau and the
// compacted list of the pairs whose lower bound does not exceed it, the search of
// sg_ged_search.h on those pairs from min(ub0, tau + 1), and per row the k' smallest
// (ub, column) with the certificate.
//
// Workspace: [count u64, pad u64][entries (m + n) * W][ub0 P][lb0 P][ub P][lb P][list P]
// [tau m][k' m], P = m * n, all int32 but the count.
#include "../../include/siamese_ged_knn.h"
#include "sg_ged_search.h"

namespace {

constexpr int kKnnMaxK = 64;
constexpr int kKnnRowThreads = 256;      // threshold and select: one workgroup per row
constexpr int kKnnBins = 1088;           // ub0 <= 64 nodes + 2 * 496 edges = 1056
constexpr int kKnnVerifyBlocks = 512;    // the verify launch: 2048 wavefronts, whatever m * n
constexpr int kKnnHead = 16;             // bytes before the entries: the candidate count

struct GedKnnArgs {
  unsigned long long *count;             // candidates listed so far
  const int32_t *ws;                     // the entries
  int32_t *ub0, *lb0, *ub, *lb;          // [m * n]
  uint32_t *list;                        // [m * n] pair indices, in any order
  int32_t *tau, *kq;                     // [m]
  int n_max, k;
  int64_t m, n, budget;
  int32_t *col_out, *ub_out, *lb_out, *cert_out, *cand_out;
  int64_t *exp_out;
};

// ---------------------------------------------------------------------------
// Seed: one wavefront per pair, sg_ged_grid's both_orders ub and lb.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGedWaves *SG_WAVE) sg_ged_knn_seed_kernel(GedKnnArgs A) {
  __shared__ GedLds lds[kGedWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t pair = (int64_t)blockIdx.x * kGedWaves + wave;
  if (pair >= A.m * A.n) return;
  const int64_t qi = pair / A.n, dj = pair - qi * A.n;
  const int nm = A.n_max, W = ged_entry_words(nm);
  const int32_t *__restrict__ e1 = A.ws + qi * W;
  const int32_t *__restrict__ e2 = A.ws + (A.m + dj) * W;
  const int n1 = __builtin_amdgcn_readfirstlane(e1[2 * nm]);
  const int n2 = __builtin_amdgcn_readfirstlane(e2[2 * nm]);
  if (n1 < 1 || n2 < 1) {   // an entry the call cannot serve
    if (lane == 0) {
      A.ub0[pair] = -1;
      A.lb0[pair] = -1;
    }
    return;
  }
  GedLds &S = lds[wave];
  uint32_t m1, m2;
  int t1, t2;
  ged_pair_load(e1, e2, nm, lane, S, m1, t1, m2, t2);
  int ub12, ub21, lb0, f12, f21;
  ged_pair_seed(n1, n2, S, lane, m1, t1, m2, t2, ub12, f12, ub21, f21, lb0);
  if (lane == 0) {
    A.ub0[pair] = ub21 < ub12 ? ub21 : ub12;
    A.lb0[pair] = lb0;
  }
}

// ---------------------------------------------------------------------------
// Threshold and filter: one workgroup per row.  A counting pass over the row's ub0 in LDS
// gives n_valid and tau; the second pass lists the candidates.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kKnnRowThreads) sg_ged_knn_threshold_kernel(GedKnnArgs A) {
  __shared__ int32_t hist[kKnnBins];
  __shared__ int32_t s_valid, s_tau, s_ncand, s_next;
  __shared__ unsigned long long s_base;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int32_t *__restrict__ ub0 = A.ub0 + row * A.n;
  const int32_t *__restrict__ lb0 = A.lb0 + row * A.n;
  for (int b = tid; b < kKnnBins; b += kKnnRowThreads) hist[b] = 0;
  if (tid == 0) {
    s_valid = 0;
    s_ncand = 0;
    s_next = 0;
  }
  __syncthreads();
  int valid = 0;
  for (int64_t j = tid; j < A.n; j += kKnnRowThreads) {
    const int u = ub0[j];
    if (u >= 0) {
      atomicAdd(&hist[u < kKnnBins ? u : kKnnBins - 1], 1);
      ++valid;
    }
  }
  if (valid) atomicAdd(&s_valid, valid);
  __syncthreads();
  if (tid == 0) {   // one walk, up to the bin that holds the k'-th smallest
    const int kq = s_valid < A.k ? s_valid : A.k;
    int tau = -1, acc = 0;
    for (int b = 0; b < kKnnBins && kq > 0; ++b) {
      acc += hist[b];
      if (acc >= kq) {
        tau = b;
        break;
      }
    }
    s_tau = tau;
    A.tau[row] = tau;
    A.kq[row] = kq;
  }
  __syncthreads();
  const int tau = s_tau;
  // the row's candidates are counted in LDS and take one range of the list: one global add
  // per row, not one per candidate
  int mine = 0;
  for (int64_t j = tid; j < A.n; j += kKnnRowThreads) mine += ub0[j] >= 0 && lb0[j] <= tau;
  if (mine) atomicAdd(&s_ncand, mine);
  __syncthreads();
  if (tid == 0) s_base = s_ncand ? atomicAdd(A.count, (unsigned long long)s_ncand) : 0ull;
  __syncthreads();
  const unsigned long long base = s_base, total = (unsigned long long)(A.m * A.n);
  for (int64_t j = tid; j < A.n; j += kKnnRowThreads) {
    if (ub0[j] >= 0 && lb0[j] <= tau) {
      const unsigned long long pos = base + (unsigned)atomicAdd(&s_next, 1);
      if (pos < total) A.list[pos] = (uint32_t)(row * A.n + j);   // always: one slot per pair
    }
  }
  if (tid == 0) {
    const bool served = A.ws[row * ged_entry_words(A.n_max) + 2 * A.n_max] >= 1;
    if (A.cand_out) A.cand_out[row] = served ? s_ncand : -1;
    if (A.exp_out) A.exp_out[row] = served ? 0 : -1;
  }
}

// ---------------------------------------------------------------------------
// Verify: a fixed launch whose wavefronts stride over the candidate list, one candidate per
// wavefront at a time.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGedWaves *SG_WAVE) sg_ged_knn_verify_kernel(GedKnnArgs A) {
  __shared__ GedExactLds lds[kGedWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  GedExactLds &X = lds[wave];
  const int nm = A.n_max, W = ged_entry_words(nm);
  const int64_t total = A.m * A.n;
  int64_t cnt = (int64_t)*A.count;
  if (cnt > total) cnt = total;
  const int64_t stride = (int64_t)kKnnVerifyBlocks * kGedWaves;
  for (int64_t i = (int64_t)blockIdx.x * kGedWaves + wave; i < cnt; i += stride) {
    const int64_t pair = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)A.list[i]);
    if (pair >= total) continue;
    const int64_t qi = pair / A.n, dj = pair - qi * A.n;
    const int32_t *__restrict__ e1 = A.ws + qi * W;
    const int32_t *__restrict__ e2 = A.ws + (A.m + dj) * W;
    const int n1 = __builtin_amdgcn_readfirstlane(e1[2 * nm]);
    const int n2 = __builtin_amdgcn_readfirstlane(e2[2 * nm]);
    const int ub0 = __builtin_amdgcn_readfirstlane(A.ub0[pair]);
    const int lb0 = __builtin_amdgcn_readfirstlane(A.lb0[pair]);
    const int tau = __builtin_amdgcn_readfirstlane(A.tau[qi]);
    int ub = ub0, lb = lb0;
    if (lb0 != ub0 && n1 >= 1 && n2 >= 1 && n1 <= kExMaxNodes && n2 <= kExMaxNodes &&
        A.budget > 0) {
      uint32_t m1, m2;
      int t1, t2;
      ged_pair_load(e1, e2, nm, lane, X.bp, m1, t1, m2, t2);
      sg_wsync();
      const int c = ub0 < tau + 1 ? ub0 : tau + 1;
      int inc = c, best = -1;
      int64_t nexp = 0;
      const bool ended = ged_search(X, n1, n2, lane, m1, t1, m2, t2, A.budget, inc, best, nexp);
      if (inc < c) {   // a complete map was found
        ub = inc;
        lb = ended ? inc : lb0;
      } else if (ended) {
        lb = c == ub0 ? ub0 : (lb0 > c ? lb0 : c);
      }
      if (A.exp_out && lane == 0) atomicAdd((unsigned long long *)(A.exp_out + qi),
                                            (unsigned long long)nexp);
      sg_wsync();   // the next candidate rewrites X
    }
    if (lane == 0) {
      A.ub[pair] = ub;
      A.lb[pair] = lb;
    }
  }
}

// minimum of a 64-bit key over the workgroup, in every thread
__device__ __forceinline__ unsigned long long knn_block_min(unsigned long long v,
                                                            unsigned long long *red,
                                                            const int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(v, o, 64);
    v = x < v ? x : v;
  }
  __syncthreads();   // red is free again
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  v = red[0];
  for (int w = 1; w < kKnnRowThreads / SG_WAVE; ++w) v = red[w] < v ? red[w] : v;
  return v;
}

// ---------------------------------------------------------------------------
// Select: one workgroup per row.  k' rounds, each the smallest (ub, column) key of the row's
// candidates above the round before's; then the certificate over the candidates left.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kKnnRowThreads) sg_ged_knn_select_kernel(GedKnnArgs A) {
  __shared__ unsigned long long red[kKnnRowThreads / SG_WAVE];
  __shared__ int32_t s_bad;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int32_t *__restrict__ ub0 = A.ub0 + row * A.n;
  const int32_t *__restrict__ lb0 = A.lb0 + row * A.n;
  const int32_t *__restrict__ ub = A.ub + row * A.n;
  const int32_t *__restrict__ lb = A.lb + row * A.n;
  const int tau = A.tau[row];
  int kq = A.kq[row];
  if (kq > A.k) kq = A.k;   // the slots that exist
  const bool served = A.ws[row * ged_entry_words(A.n_max) + 2 * A.n_max] >= 1;
  const unsigned long long none = ~0ull;
  if (tid == 0) s_bad = 0;
  unsigned long long last = 0;
  int unproven = 0;   // thread 0's: a selected pair with lb != ub
  for (int r = 0; r < kq; ++r) {
    unsigned long long best = none;
    for (int64_t j = tid; j < A.n; j += kKnnRowThreads) {
      if (ub0[j] >= 0 && lb0[j] <= tau) {
        const unsigned long long key = ((unsigned long long)(uint32_t)ub[j] << 32) | (uint32_t)j;
        if ((r == 0 || key > last) && key < best) best = key;
      }
    }
    best = knn_block_min(best, red, tid);
    const int64_t j = best == none ? -1 : (int64_t)(best & 0xFFFFFFFFull);
    if (tid == 0) {
      const int64_t o = row * A.k + r;
      A.col_out[o] = (int32_t)j;
      A.ub_out[o] = j < 0 ? -1 : ub[j];
      A.lb_out[o] = j < 0 ? -1 : lb[j];
      if (j < 0 || lb[j] != ub[j]) unproven = 1;
    }
    last = best;
  }
  for (int r = kq + tid; r < A.k; r += kKnnRowThreads) {
    const int64_t o = row * A.k + r;
    A.col_out[o] = -1;
    A.ub_out[o] = -1;
    A.lb_out[o] = -1;
  }
  // every candidate left must lie behind the last selected one, by (lb, column)
  int bad = 0;
  const int d = (int)(last >> 32);
  const int64_t s = (int64_t)(last & 0xFFFFFFFFull);
  for (int64_t j = tid; j < A.n && kq > 0; j += kKnnRowThreads) {
    if (ub0[j] >= 0 && lb0[j] <= tau) {
      const unsigned long long key = ((unsigned long long)(uint32_t)ub[j] << 32) | (uint32_t)j;
      if (key > last && !(lb[j] > d || (lb[j] == d && j > s))) bad = 1;
    }
  }
  __syncthreads();   // s_bad is zero
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  if (tid == 0) A.cert_out[row] = served && !unproven && !s_bad ? 1 : 0;
}

int ged_knn_rc(int64_t m, int64_t n, int32_t n_max, int32_t k) {
  const int rc = ged_shape_rc(m, n, n_max);
  if (rc != SG_OK) return rc;
  if (k < 1) return SG_ERR_ARG;
  if (k > kKnnMaxK) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

}  // namespace

extern "C" {

int64_t sg_ged_knn_workspace_bytes(int64_t m, int64_t n, int32_t n_max, int32_t k) {
  if (ged_knn_rc(m, n, n_max, k) != SG_OK) return -1;
  if (m == 0 || n == 0) return 0;
  return kKnnHead + 4 * ((m + n) * (int64_t)ged_entry_words(n_max) + 5 * m * n + 2 * m);
}

int32_t sg_ged_knn(const float *store_adj, const int32_t *store_types, const int32_t *store_n,
                   int32_t n_graphs, int32_t n_max, const int32_t *q_idx, int64_t m,
                   const int32_t *db_idx, int64_t n, int32_t k, int64_t max_expansions,
                   int32_t *col_out, int32_t *ub_out, int32_t *lb_out, int32_t *certified_out,
                   int32_t *candidates_out, int64_t *expansions_out, int32_t *status_out,
                   void *workspace, sg_stream_t stream) {
  if (m < 0 || n < 0) return SG_ERR_ARG;
  if (n_graphs < 0) return SG_ERR_ARG;
  const int rc = ged_knn_rc(m, n, n_max, k);
  if (rc != SG_OK) return rc;
  if (max_expansions < 0) return SG_ERR_ARG;
  if (max_expansions > kExMaxBudget) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !col_out || !ub_out || !lb_out ||
      !certified_out || !workspace)
    return SG_ERR_ARG;
  if ((uintptr_t)workspace & 7) return SG_ERR_ARG;   // the 64-bit candidate count
  hipStream_t st = (hipStream_t)stream;
  const int64_t P = m * n;
  GedKnnArgs G;
  G.count = (unsigned long long *)workspace;
  int32_t *w = (int32_t *)((char *)workspace + kKnnHead);
  G.ws = w;
  w += (m + n) * (int64_t)ged_entry_words(n_max);
  G.ub0 = w;
  G.lb0 = w + P;
  G.ub = w + 2 * P;
  G.lb = w + 3 * P;
  G.list = (uint32_t *)(w + 4 * P);
  G.tau = w + 5 * P;
  G.kq = w + 5 * P + m;
  G.n_max = n_max;
  G.k = k;
  G.m = m;
  G.n = n;
  G.budget = max_expansions;
  G.col_out = col_out;
  G.ub_out = ub_out;
  G.lb_out = lb_out;
  G.cert_out = certified_out;
  G.cand_out = candidates_out;
  G.exp_out = expansions_out;
  if (hipMemsetAsync(workspace, 0, kKnnHead, st) != hipSuccess) return SG_ERR_HIP;
  ged_launch_prep(store_adj, store_types, store_n, n_graphs, n_max, q_idx, m, db_idx, n,
                  status_out, (void *)G.ws, st);
  hipLaunchKernelGGL(sg_ged_knn_seed_kernel, dim3((unsigned)((P + kGedWaves - 1) / kGedWaves)),
                     dim3(kGedWaves * SG_WAVE), 0, st, G);
  hipLaunchKernelGGL(sg_ged_knn_threshold_kernel, dim3((unsigned)m), dim3(kKnnRowThreads), 0, st,
                     G);
  hipLaunchKernelGGL(sg_ged_knn_verify_kernel, dim3(kKnnVerifyBlocks), dim3(kGedWaves * SG_WAVE),
                     0, st, G);
  hipLaunchKernelGGL(sg_ged_knn_select_kernel, dim3((unsigned)m), dim3(kKnnRowThreads), 0, st,
                     G);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
