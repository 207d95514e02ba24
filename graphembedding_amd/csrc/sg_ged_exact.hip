// sg_ged_exact.hip — exact graph edit distance under an expansion budget for every pair of a
// query x database grid (include/siamese_ged_exact.h): a depth-first branch and bound over
// node maps, seeded with the bipartite bounds of sg_ged_common.h.  Two launches per call: the
// m + n entries' adjacency bit masks into the workspace (sg_ged.hip's), then one wavefront
// per pair.
//
// Lane mapping: lane j < n2 is graph-2 node j, lane n2 is epsilon; an expansion computes the
// step cost, h and f of all n2 + 1 <= 17 children at once, each in its lane.  The partial map
// lives in the lanes as psi (the graph-1 node mapped to this lane's graph-2 node, or -1), so
// the set of used graph-2 nodes and the images of node k's mapped neighbours are one ballot
// each.  All control flow is wave-uniform: depth, g, the incumbent and the expansion count are
// scalars.  Per level the children's keys f << 14 | j << 9 | h stay in LDS; the next child of
// a level is the smallest key above the level's last one (a 16-lane DPP minimum plus the
// epsilon lane), which visits them in ascending (f, j) without a sort.
#include "../../include/siamese_ged_exact.h"
#include "sg_ged_common.h"

namespace {

constexpr int kExMaxNodes = 16;                      // the search serves max(n1, n2) <= 16
constexpr int kExLanes = kExMaxNodes + 1;            // children of a state: n2 nodes + epsilon
constexpr int64_t kExMaxBudget = (int64_t)1 << 24;   // max_expansions
constexpr int kExNone = 0x7FFFFFFF;                  // no child: above every key

struct GedExactArgs {
  const int32_t *ws;
  int n_max;
  int64_t m, n, ld, budget;
  int32_t *ub, *lb;
  int8_t *map;    // or null
  int64_t *exp;   // or null
};

// the wavefront's LDS: the seed's, then per level the children's keys and (I | EU << 8) of the
// child state, the key taken last, and per graph-1 node k the masks of the graph-1 / graph-2
// nodes of its type and the edges of E1 with an end above k
struct GedExactLds {
  GedLds bp;
  int32_t key[kExMaxNodes][kExLanes];
  int32_t aux[kExMaxNodes][kExLanes];
  int32_t last[kExMaxNodes];
  uint32_t T1[kExMaxNodes], T2[kExMaxNodes];
  int32_t pd[kExMaxNodes], e1r[kExMaxNodes];
};

__device__ __forceinline__ int ged_imin(int a, int b) { return a < b ? a : b; }

// minimum over lanes 0 .. 16 as a scalar: rows 0 and 1 each reduce over their 16 lanes (quad
// swaps, then the mirrored half and row), lanes 17 .. 31 hold kExNone
__device__ __forceinline__ int ged_min17(int v) {
  v = ged_imin(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm 1,0,3,2
  v = ged_imin(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm 2,3,0,1
  v = ged_imin(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = ged_imin(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
  return ged_imin(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
}

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
  // the seed: both assignment orders and the lower bound, as sg_ged_grid computes them
  int p, f12, f21;
  ged_lsap(n1, n2, 1, S.t[0], S.deg[0], t2, d2, S.u, lane, p);   // its entry fence covers S
  const int ub12 = __builtin_amdgcn_readfirstlane(
      ged_induced(n1, n2, p, t1, m1, S.t[1], S.mask[1], S.phi, sumdeg, lane, f12));
  ged_lsap(n2, n1, 1, S.t[1], S.deg[1], t1, d1, S.u, lane, p);
  const int ub21 = __builtin_amdgcn_readfirstlane(
      ged_induced(n2, n1, p, t2, m2, S.t[0], S.mask[0], S.phi, sumdeg, lane, f21));
  const int lb0 = __builtin_amdgcn_readfirstlane(
      (ged_lsap(n1, n2, 2, S.t[0], S.deg[0], t2, d2, S.u, lane, p) + 1) >> 1);
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

  if (!proven && n1 <= kExMaxNodes && n2 <= kExMaxNodes && A.budget > 0) {
    // per graph-1 node the nodes of its type on both sides; per lane those of this lane's
    // graph-2 node's type
    uint32_t K1 = 0, K2 = 0;
    for (int a = 0; a < n1; ++a) {
      const int x = S.t[0][a];
      const uint32_t s1 = (uint32_t)__ballot(lane < n1 && t1 == x);
      const uint32_t s2 = (uint32_t)__ballot(lane < n2 && t2 == x);
      if (lane == 0) {
        X.T1[a] = s1;
        X.T2[a] = s2;
      }
    }
    for (int b = 0; b < n2; ++b) {
      const int x = S.t[1][b];
      const uint32_t s1 = (uint32_t)__ballot(lane < n1 && t1 == x);
      const uint32_t s2 = (uint32_t)__ballot(lane < n2 && t2 == x);
      if (lane == b) {
        K1 = s1;
        K2 = s2;
      }
    }
    const uint32_t below = lane < 32 ? (1u << lane) - 1u : 0xFFFFFFFFu;
    if (lane < kExMaxNodes) X.pd[lane] = lane < n1 ? __popc(m1 & below) : 0;
    sg_wsync();
    int I = 0;   // |multiset intersection| of all types: each type at its first graph-1 node
    if (lane < n1) {
      int s = 0;
      for (int a = 0; a < n1; ++a) s += a > lane ? X.pd[a] : 0;
      X.e1r[lane] = s;
      const uint32_t own1 = X.T1[lane], own2 = X.T2[lane];
      if ((own1 & below) == 0) I = ged_imin(__popc(own1), __popc(own2));
    }
    I = __builtin_amdgcn_readfirstlane(ged_wave_sum(I));
    const int E2 = __builtin_amdgcn_readfirstlane(ged_wave_sum(d2)) >> 1;
    sg_wsync();

    int psi = -1;   // the graph-1 node mapped to this lane's graph-2 node
    int k = 0, g = 0, EU = 0;   // depth, cost so far, edges of E2 among the used nodes
    int expand = 1;
    const int64_t steps = A.budget * (kExLanes + 3) + 4;   // an expansion, <= 17 children, a return
    for (int64_t it = 0; it < steps; ++it) {
      // the search state is the same in every lane: keep it in scalar registers
      k = __builtin_amdgcn_readfirstlane(k);
      g = __builtin_amdgcn_readfirstlane(g);
      I = __builtin_amdgcn_readfirstlane(I);
      EU = __builtin_amdgcn_readfirstlane(EU);
      inc = __builtin_amdgcn_readfirstlane(inc);
      expand = __builtin_amdgcn_readfirstlane(expand);
      if (expand) {
        if (nexp == A.budget) break;
        ++nexp;
        const uint32_t used = (uint32_t)__ballot(psi >= 0);
        const uint32_t m1k = S.mask[0][k], low = (1u << k) - 1u;
        const uint32_t img = (uint32_t)__ballot(psi >= 0 && ((m1k >> (psi & 31)) & 1u));
        const int nb = __popc(m1k & low), dele = nb - __popc(img);
        const int Ik = I - (__popc(X.T1[k] & ~low) <= __popc(X.T2[k] & ~used) ? 1 : 0);
        const int r1 = n1 - k - 1, r2 = n2 - __popc(used);
        const bool sub = lane < n2 && psi < 0, eps = lane == n2;
        int keyv = kExNone, auxv = 0;
        if (sub || eps) {
          const int c = sub ? (S.t[0][k] != t2 ? 1 : 0) + __popc(img ^ (m2 & used)) + dele
                            : 1 + nb;
          const int Ic =
              Ik - (sub && __popc(K2 & ~used) <= __popc(K1 & ~(low | (1u << k))) ? 1 : 0);
          const int EUc = EU + (sub ? __popc(m2 & used) : 0);
          const int r2c = r2 - (sub ? 1 : 0);
          const int h = (r1 > r2c ? r1 : r2c) - Ic + abs(X.e1r[k] - (E2 - EUc));
          keyv = ((g + c + h) << 14) | (lane << 9) | h;
          auxv = Ic | (EUc << 8);
        }
        if (lane < kExLanes) {
          X.key[k][lane] = keyv;
          X.aux[k][lane] = auxv;
        }
        if (lane == 0) X.last[k] = -1;
        sg_wsync();
        expand = 0;
        continue;
      }
      const int lastk = X.last[k];
      int kv = lane < kExLanes ? X.key[k][lane] : kExNone;
      if (kv <= lastk) kv = kExNone;
      const int mn = ged_min17(kv);
      const int f = mn >> 14;
      if (mn == kExNone || f >= inc) {   // the level is done
        if (k == 0) {
          proven = true;
          break;
        }
        --k;
        if (psi == k) psi = -1;
        continue;
      }
      const int c = (mn >> 9) & 31;
      if (lane == 0) X.last[k] = mn;
      sg_wsync();
      if (k == n1 - 1) {   // a complete map: f is its cost
        inc = f;
        best = lane == c && c < n2 ? k : psi;
        continue;
      }
      if (lane == c && c < n2) psi = k;
      const int ax = __builtin_amdgcn_readfirstlane(X.aux[k][c]);
      g = f - (mn & 511);
      I = ax & 255;
      EU = ax >> 8;
      ++k;
      expand = 1;
    }
  }

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
