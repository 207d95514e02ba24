// sg_ged_common.h — what the graph edit distance units share (sg_ged.hip: the bipartite
// bounds of include/siamese_ged.h; sg_ged_exact.hip and sg_ged_beam.hip: the budgeted search of
// include/siamese_ged_exact.h and the beam search of include/siamese_ged_beam.h that those
// bounds seed): the workspace entry of a graph and the
// kernel that builds it, the wave-wide assignment solver and the cost of the edit path an
// assignment induces, and the rules on m, n and n_max.
#pragma once
#include "sg_common.h"

namespace {

constexpr int kGedMaxNodes = 32;                    // N = n1 + n2 <= 64: one lane per column
constexpr int64_t kGedMaxSide = (int64_t)1 << 24;   // m, n
constexpr int64_t kGedMaxPairs = (int64_t)1 << 32;  // m * n: one wavefront per pair
constexpr int kGedWaves = 4;                        // wavefronts (pairs) per workgroup
constexpr int kGedBig = 1 << 20;                    // forbidden entries: far above any path
constexpr int kGedInf = 0x7FFFFFFF;                 // minv before a row's first round

// workspace entry of one graph, in 4-byte words: [n_max] adjacency row masks (bit b of word a:
// nodes a != b share an edge), [n_max] types, then the node count, or -1 for an entry that
// cannot be served
__host__ __device__ inline int ged_entry_words(int n_max) { return (2 * n_max + 1 + 3) & ~3; }

struct GedPrepArgs {
  const float *sadj;
  const int32_t *stypes, *sn;
  int n_graphs, n_max;
  const int32_t *qidx, *dbidx;   // or null: entry k is graph k
  int64_t m, total;              // entries [0, m) are queries, [m, total) database graphs
  int32_t *ws;
  int32_t *status;
};

// the wavefront's LDS: both graphs' types, degrees and row masks by node, the solver's row
// potentials and the assignment by row
struct GedLds {
  int32_t t[2][kGedMaxNodes];
  int32_t deg[2][kGedMaxNodes];
  uint32_t mask[2][kGedMaxNodes];
  int32_t u[SG_WAVE];
  int32_t phi[kGedMaxNodes];
};

__device__ __forceinline__ int ged_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// minimum of a packed (value << 6 | column) key over the wavefront, as a scalar: the smallest
// value, and among equal values the smallest column
__device__ __forceinline__ uint32_t ged_wave_min(uint32_t k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = __shfl_xor(k, o, 64);
    k = x < k ? x : k;
  }
  return __builtin_amdgcn_readfirstlane(k);
}

// ---------------------------------------------------------------------------
// One wavefront per entry: lane a builds the mask of node a's row.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGedWaves *SG_WAVE) sg_ged_prep_kernel(GedPrepArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t e = (int64_t)blockIdx.x * kGedWaves + wave;
  if (e >= A.total) return;
  const bool isq = e < A.m;
  const int64_t k = isq ? e : e - A.m;
  const int32_t *idx = isq ? A.qidx : A.dbidx;
  const int64_t id = idx ? (int64_t)idx[k] : k;
  const bool in_store = id >= 0 && id < A.n_graphs;
  const int nm = A.n_max;
  const int n = in_store ? A.sn[id] : 0;
  int32_t *dst = A.ws + e * ged_entry_words(nm);
  if (!(in_store && n >= 1 && n <= nm)) {
    if (lane == 0) {
      if (A.status) atomicExch(A.status, (int32_t)(in_store ? SG_ERR_SHAPE : SG_ERR_ARG));
      dst[2 * nm] = -1;
    }
    return;
  }
  if (lane < nm) {
    uint32_t mask = 0;
    int t = 0;
    if (lane < n) {
      const float *__restrict__ row = A.sadj + (id * nm + lane) * nm;
      for (int b = 0; b < n; ++b)
        if (b != lane && row[b] != 0.f) mask |= 1u << b;
      t = A.stypes[id * nm + lane];
    }
    dst[lane] = (int32_t)mask;
    dst[nm + lane] = t;
  }
  if (lane == 0) dst[2 * nm] = n;
}

// the m + n entries of a call into its workspace
inline void ged_launch_prep(const float *store_adj, const int32_t *store_types,
                            const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                            const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                            int32_t *status_out, void *workspace, hipStream_t stream) {
  GedPrepArgs P;
  P.sadj = store_adj;
  P.stypes = store_types;
  P.sn = store_n;
  P.n_graphs = n_graphs;
  P.n_max = n_max;
  P.qidx = q_idx;
  P.dbidx = db_idx;
  P.m = m;
  P.total = m + n;
  P.ws = (int32_t *)workspace;
  P.status = status_out;
  hipLaunchKernelGGL(sg_ged_prep_kernel, dim3((unsigned)((m + n + kGedWaves - 1) / kGedWaves)),
                     dim3(kGedWaves * SG_WAVE), 0, stream, P);
}

// ---------------------------------------------------------------------------
// The assignment problem of nr row nodes against nc column nodes, N = nr + nc <= 64, on the
// matrix of siamese_ged.h with substitution weight w.  Lane c owns column c: its potential v,
// minv, way and the row p assigned to it stay in registers; the entry C[row][c] is computed
// from the broadcast row's (type, degree) and the lane's own column (ct, cdeg), so no matrix
// is stored.  Row potentials live in u[N] (LDS).  Rows enter in index order; a round takes
// the unused column of smallest minv (ties: smallest index) as one wave-wide minimum of
// minv << 6 | c (reduced costs are never negative) and marks it, so a row needs at most N
// rounds.  Returns the optimum Σu + Σv; p_out is the row of this lane's column.
// ---------------------------------------------------------------------------
__device__ int ged_lsap(const int nr, const int nc, const int w, const int32_t *rt,
                        const int32_t *rdeg, const int ct, const int cdeg, int32_t *u,
                        const int lane, int &p_out) {
  const int N = nr + nc;
  const bool live = lane < N, creal = lane < nc;
  int v = 0, p = -1;
  u[lane] = 0;
  sg_wsync();
  for (int i = 0; i < N; ++i) {
    int minv = kGedInf, way = -1;
    bool used = !live;
    int ui = 0;            // u[i]: row i is assigned to no column until the augmentation
    int j0 = -1, i0 = i;   // the column marked last (-1: none yet) and its row
    int u0 = 0;
    for (int r = 0; r < N; ++r) {
      int cost;
      if (i0 < nr) {
        const int t = rt[i0], d = rdeg[i0];
        cost = creal ? w * (t != ct ? 1 : 0) + abs(d - cdeg) : (lane - nc == i0 ? w + d : kGedBig);
      } else {
        cost = creal ? (i0 - nr == lane ? w + cdeg : kGedBig) : 0;
      }
      const int cur = cost - u0 - v;
      if (!used && cur < minv) {
        minv = cur;
        way = j0;
      }
      const uint32_t key =
          ged_wave_min(used ? 0xFFFFFFFFu : (((uint32_t)minv << 6) | (uint32_t)lane));
      const int j1 = (int)(key & 63u), delta = (int)(key >> 6);
      if (used) {
        if (live) {   // a marked column is an assigned one
          v -= delta;
          u[p] += delta;
        }
      } else {
        minv -= delta;
      }
      ui += delta;
      j0 = j1;
      used = used || lane == j0;
      i0 = __builtin_amdgcn_readlane(p, j0);
      if (i0 < 0) break;   // a free column: the path ends
      sg_wsync();
      u0 = u[i0];
    }
    for (int r = 0; r < N && j0 >= 0; ++r) {   // flip the path back to row i
      const int j1 = __builtin_amdgcn_readlane(way, j0);
      const int pj = __builtin_amdgcn_readlane(p, j1 & 63);
      if (lane == j0) p = j1 < 0 ? i : pj;
      j0 = j1;
    }
    if (lane == 0) u[i] = ui;
    sg_wsync();
  }
  p_out = p;
  return ged_wave_sum(live ? u[lane] + v : 0);
}

// The cost of the edit path of an assignment (p: the row of this lane's column), rows = the
// graph whose node `lane` has type my_t and row mask my_mask, columns = the graph of ot /
// omask.  sumdeg = 2 (|E1| + |E2|).  phi_out: the column node of row node `lane`, or -1.
__device__ int ged_induced(const int nr, const int nc, const int p, const int my_t,
                           const uint32_t my_mask, const int32_t *ot, const uint32_t *omask,
                           int32_t *phi, const int sumdeg, const int lane, int &phi_out) {
  if (lane < nr + nc && p >= 0 && p < nr) phi[p] = lane < nc ? lane : -1;
  sg_wsync();
  const int f = lane < nr ? phi[lane] : -1;
  uint32_t img = 0;   // the images of this node's neighbours
  for (int b = 0; b < nr; ++b) {
    const int fb = phi[b];
    if (fb >= 0 && ((my_mask >> b) & 1u)) img |= 1u << fb;
  }
  const bool del = lane < nr && f < 0;
  int local = 0;   // type mismatch, minus the kept edges at this node (each edge at both ends)
  if (lane < nr && f >= 0) local = (my_t != ot[f] ? 1 : 0) - __popc(img & omask[f]);
  const int dels = __popcll(__ballot(del));
  const int s = ged_wave_sum(local);
  sg_wsync();   // phi is rewritten by the next order
  phi_out = f;
  return dels + (nc - nr + dels) + s + sumdeg / 2;
}

// the rules on m, n and n_max alone (siamese_ged.h, in its order)
inline int ged_shape_rc(int64_t m, int64_t n, int32_t n_max) {
  if (m < 0 || n < 0) return SG_ERR_ARG;
  if (n_max < 1) return SG_ERR_ARG;
  if (n_max > kGedMaxNodes) return SG_ERR_UNSUPPORTED;
  if (m > kGedMaxSide || n > kGedMaxSide || m * n > kGedMaxPairs) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

}  // namespace
