// sg_ged.hip — graph edit distance bounds for every pair of a query x database grid
// (include/siamese_ged.h): the bipartite approximation of Riesen & Bunke.  Per pair one
// linear sum assignment problem on the (n1 + n2)² integer matrix of node edits with their
// local edge costs, the edit path its assignment induces (upper bound) and the same problem
// on the half-edge-cost matrix (lower bound).  Two launches per call: the m + n entries'
// adjacency bit masks into the workspace, then one wavefront per pair.
// The entry builder, the solver and the induced cost are sg_ged_common.h's: the budgeted search
// of sg_ged_exact.hip seeds its incumbent with them.
#include "../../include/siamese_ged.h"
#include "sg_ged_common.h"

namespace {

struct GedGridArgs {
  const int32_t *ws;
  int n_max, both;
  int64_t m, n, ld;
  int32_t *ub, *lb;   // lb or null
  int8_t *map;        // or null
};

// ---------------------------------------------------------------------------
// One wavefront per pair (i, j) of the grid.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGedWaves *SG_WAVE) sg_ged_grid_kernel(GedGridArgs A) {
  __shared__ GedLds lds[kGedWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t pair = (int64_t)blockIdx.x * kGedWaves + wave;
  if (pair >= A.m * A.n) return;
  const int64_t qi = pair / A.n, dj = pair - qi * A.n;
  const int nm = A.n_max, W = ged_entry_words(nm);
  const int32_t *__restrict__ e1 = A.ws + qi * W;
  const int32_t *__restrict__ e2 = A.ws + (A.m + dj) * W;
  const int n1 = e1[2 * nm], n2 = e2[2 * nm];
  const int64_t o = qi * A.ld + dj;
  int8_t *map = A.map ? A.map + pair * nm : nullptr;
  if (n1 < 1 || n2 < 1) {   // an entry the call cannot serve
    if (lane == 0) {
      A.ub[o] = -1;
      if (A.lb) A.lb[o] = -1;
    }
    if (map && lane < nm) map[lane] = -1;
    return;
  }
  GedLds &S = lds[wave];
  uint32_t m1 = 0, m2 = 0;
  int t1 = 0, t2 = 0;
  if (lane < nm) {
    m1 = (uint32_t)e1[lane];
    t1 = e1[nm + lane];
    m2 = (uint32_t)e2[lane];
    t2 = e2[nm + lane];
  }
  const int d1 = __popc(m1), d2 = __popc(m2);
  if (lane < kGedMaxNodes) {
    S.t[0][lane] = t1;
    S.deg[0][lane] = d1;
    S.mask[0][lane] = m1;
    S.t[1][lane] = t2;
    S.deg[1][lane] = d2;
    S.mask[1][lane] = m2;
  }
  const int sumdeg = ged_wave_sum(d1 + d2);
  int p, f;
  ged_lsap(n1, n2, 1, S.t[0], S.deg[0], t2, d2, S.u, lane, p);   // its entry fence covers S
  int ub = ged_induced(n1, n2, p, t1, m1, S.t[1], S.mask[1], S.phi, sumdeg, lane, f);
  if (map && lane < nm) map[lane] = (int8_t)f;
  if (A.both) {
    int f2;
    ged_lsap(n2, n1, 1, S.t[1], S.deg[1], t1, d1, S.u, lane, p);
    const int ub2 = ged_induced(n2, n1, p, t2, m2, S.t[0], S.mask[0], S.phi, sumdeg, lane, f2);
    ub = ub2 < ub ? ub2 : ub;
  }
  if (lane == 0) A.ub[o] = ub;
  if (A.lb) {
    const int opt = ged_lsap(n1, n2, 2, S.t[0], S.deg[0], t2, d2, S.u, lane, p);
    if (lane == 0) A.lb[o] = (opt + 1) >> 1;
  }
}

}  // namespace

extern "C" {

int64_t sg_ged_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max) {
  if (ged_shape_rc(m, n, n_max) != SG_OK) return -1;
  if (m == 0 || n == 0) return 0;
  return (m + n) * (int64_t)ged_entry_words(n_max) * 4;
}

int32_t sg_ged_grid(const float *store_adj, const int32_t *store_types, const int32_t *store_n,
                    int32_t n_graphs, int32_t n_max, const int32_t *q_idx, int64_t m,
                    const int32_t *db_idx, int64_t n, int32_t both_orders, int32_t *ub_out,
                    int64_t ld, int32_t *lb_out, int8_t *map_out, int32_t *status_out,
                    void *workspace, sg_stream_t stream) {
  if (m < 0 || n < 0 || ld < 0) return SG_ERR_ARG;
  if (n_graphs < 0) return SG_ERR_ARG;
  const int rc = ged_shape_rc(m, n, n_max);
  if (rc != SG_OK) return rc;
  if (ld < n) return SG_ERR_ARG;
  if (both_orders != 0 && both_orders != 1) return SG_ERR_ARG;
  if (m == 0 || n == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !ub_out || !workspace) return SG_ERR_ARG;
  ged_launch_prep(store_adj, store_types, store_n, n_graphs, n_max, q_idx, m, db_idx, n,
                  status_out, workspace, (hipStream_t)stream);
  GedGridArgs G;
  G.ws = (const int32_t *)workspace;
  G.n_max = n_max;
  G.both = both_orders;
  G.m = m;
  G.n = n;
  G.ld = ld;
  G.ub = ub_out;
  G.lb = lb_out;
  G.map = map_out;
  hipLaunchKernelGGL(sg_ged_grid_kernel, dim3((unsigned)((m * n + kGedWaves - 1) / kGedWaves)),
                     dim3(kGedWaves * SG_WAVE), 0, (hipStream_t)stream, G);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
