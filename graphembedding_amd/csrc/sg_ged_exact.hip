// sg_ged_exact.hip — exact graph edit distance under an expansion budget for every pair of a
// query x database grid (include/siamese_ged_exact.h): a depth-first branch and bound over
// node maps, seeded with the bipartite bounds of sg_ged_common.h.  Two launches per call: the
// m + n entries' adjacency bit masks into the workspace (sg_ged.hip's), then one wavefront
// per pair.
//
// Lane mapping and search: sg_ged_search.h, which sg_ged_knn.hip shares.
#include "../../include/siamese_ged_exact.h"
#include "sg_ged_search.h"

namespace {

struct GedExactArgs {
  const int32_t *ws;
  int n_max;
  int64_t m, n, ld, budget;
  int32_t *ub, *lb;
  int8_t *map;    // or null
  int64_t *exp;   // or null
};

// ---------------------------------------------------------------------------
// One wavefront per pair (i, j) of the grid.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGedWaves *SG_WAVE) sg_ged_exact_kernel(GedExactArgs A) {
  __shared__ GedExactLds lds[kGedWaves];
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
  const int64_t o = qi * A.ld + dj;
  int8_t *map = A.map ? A.map + pair * nm : nullptr;
  if (n1 < 1 || n2 < 1) {   // an entry the call cannot serve
    if (lane == 0) {
      A.ub[o] = -1;
      A.lb[o] = -1;
      if (A.exp) A.exp[o] = -1;
    }
    if (map && lane < nm) map[lane] = -1;
    return;
  }
  GedExactLds &X = lds[wave];
  GedLds &S = X.bp;
  uint32_t m1, m2;
  int t1, t2;
  ged_pair_load(e1, e2, nm, lane, S, m1, t1, m2, t2);
  // the seed: both assignment orders and the lower bound, as sg_ged_grid computes them
  int ub12, ub21, lb0, f12, f21;
  ged_pair_seed(n1, n2, S, lane, m1, t1, m2, t2, ub12, f12, ub21, f21, lb0);
  // the incumbent's map by graph-2 node: f21 is one already, f12 is turned round in LDS
  if (lane < kGedMaxNodes) S.phi[lane] = -1;
  sg_wsync();
  if (lane < n1 && f12 >= 0) S.phi[f12] = lane;
  sg_wsync();
  const int inv12 = lane < kGedMaxNodes ? S.phi[lane] : -1;
  sg_wsync();
  int best = ub21 < ub12 ? f21 : inv12;
  int inc = ub21 < ub12 ? ub21 : ub12;
  int64_t nexp = 0;
  bool proven = lb0 == inc;
  if (!proven && n1 <= kExMaxNodes && n2 <= kExMaxNodes && A.budget > 0)
    proven = ged_search(X, n1, n2, lane, m1, t1, m2, t2, A.budget, inc, best, nexp);

  if (lane == 0) {
    A.ub[o] = inc;
    A.lb[o] = proven ? inc : lb0;
    if (A.exp) A.exp[o] = nexp;
  }
  if (map) {
    if (lane < kGedMaxNodes) S.phi[lane] = -1;
    sg_wsync();
    if (lane < n2 && best >= 0) S.phi[best] = lane;
    sg_wsync();
    if (lane < nm) map[lane] = (int8_t)(lane < n1 ? S.phi[lane] : -1);
  }
}

}  // namespace

extern "C" {

int64_t sg_ged_exact_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max) {
  if (ged_shape_rc(m, n, n_max) != SG_OK) return -1;
  if (m == 0 || n == 0) return 0;
  return (m + n) * (int64_t)ged_entry_words(n_max) * 4;
}

int32_t sg_ged_exact_grid(const float *store_adj, const int32_t *store_types,
                          const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                          const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                          int64_t max_expansions, int32_t *ub_out, int64_t ld, int32_t *lb_out,
                          int8_t *map_out, int64_t *expansions_out, int32_t *status_out,
                          void *workspace, sg_stream_t stream) {
  if (m < 0 || n < 0 || ld < 0) return SG_ERR_ARG;
  if (n_graphs < 0) return SG_ERR_ARG;
  const int rc = ged_shape_rc(m, n, n_max);
  if (rc != SG_OK) return rc;
  if (ld < n) return SG_ERR_ARG;
  if (max_expansions < 0) return SG_ERR_ARG;
  if (max_expansions > kExMaxBudget) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !ub_out || !lb_out || !workspace)
    return SG_ERR_ARG;
  ged_launch_prep(store_adj, store_types, store_n, n_graphs, n_max, q_idx, m, db_idx, n,
                  status_out, workspace, (hipStream_t)stream);
  GedExactArgs G;
  G.ws = (const int32_t *)workspace;
  G.n_max = n_max;
  G.m = m;
  G.n = n;
  G.ld = ld;
  G.budget = max_expansions;
  G.ub = ub_out;
  G.lb = lb_out;
  G.map = map_out;
  G.exp = expansions_out;
  hipLaunchKernelGGL(sg_ged_exact_kernel, dim3((unsigned)((m * n + kGedWaves - 1) / kGedWaves)),
                     dim3(kGedWaves * SG_WAVE), 0, (hipStream_t)stream, G);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
