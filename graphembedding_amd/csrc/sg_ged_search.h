// sg_ged_search.h — the depth-first branch and bound of include/siamese_ged_exact.h as device
// code, shared by sg_ged_exact.hip (every pair of a grid, from the bipartite incumbent) and
// sg_ged_knn.hip (the pairs that survive a row's filter, from a cutoff): the wavefront's LDS,
// the bipartite seed, and the search from a given incumbent.
//
// Lane mapping: lane j < n2 is graph-2 node j, lane n2 is epsilon; an expansion computes the
// step cost, h and f of all n2 + 1 <= 17 children at once, each in its lane.  The partial map
// lives in the lanes as psi (the graph-1 node mapped to this lane's graph-2 node, or -1), so
// the set of used graph-2 nodes and the images of node k's mapped neighbours are one ballot
// each.  All control flow is wave-uniform: depth, g, the incumbent and the expansion count are
// scalars.  Per level the children's keys f << 14 | j << 9 | h stay in LDS; the next child of
// a level is the smallest key above the level's last one (a 16-lane DPP minimum plus the
// epsilon lane), which visits them in ascending (f, j) without a sort.
#pragma once
#include "sg_ged_common.h"

namespace {

constexpr int kExMaxNodes = 16;                      // the search serves max(n1, n2) <= 16
constexpr int kExLanes = kExMaxNodes + 1;            // children of a state: n2 nodes + epsilon
constexpr int64_t kExMaxBudget = (int64_t)1 << 24;   // max_expansions
constexpr int kExNone = 0x7FFFFFFF;                  // no child: above every key

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

// Both graphs of a pair from their workspace entries: lane a's row mask and type of node a on
// either side in registers, and types, degrees and masks by node in S.  A caller that reads S
// before the next ged_lsap (whose entry fence covers it) fences first.
__device__ __forceinline__ void ged_pair_load(const int32_t *__restrict__ e1,
                                              const int32_t *__restrict__ e2, const int nm,
                                              const int lane, GedLds &S, uint32_t &m1, int &t1,
                                              uint32_t &m2, int &t2) {
  m1 = 0, m2 = 0, t1 = 0, t2 = 0;
  if (lane < nm) {
    m1 = (uint32_t)e1[lane];
    t1 = e1[nm + lane];
    m2 = (uint32_t)e2[lane];
    t2 = e2[nm + lane];
  }
  if (lane < kGedMaxNodes) {
    S.t[0][lane] = t1;
    S.deg[0][lane] = __popc(m1);
    S.mask[0][lane] = m1;
    S.t[1][lane] = t2;
    S.deg[1][lane] = __popc(m2);
    S.mask[1][lane] = m2;
  }
}

// The seed of a loaded pair: both assignment orders' upper bounds with their maps (f12: the
// graph-2 node of graph-1 node `lane`; f21: the graph-1 node of graph-2 node `lane`) and the
// lower bound, as sg_ged_grid computes them.
__device__ __forceinline__ void ged_pair_seed(const int n1, const int n2, GedLds &S,
                                              const int lane, const uint32_t m1, const int t1,
                                              const uint32_t m2, const int t2, int &ub12,
                                              int &f12, int &ub21, int &f21, int &lb0) {
  const int d1 = __popc(m1), d2 = __popc(m2);
  const int sumdeg = ged_wave_sum(d1 + d2);
  int p;
  ged_lsap(n1, n2, 1, S.t[0], S.deg[0], t2, d2, S.u, lane, p);   // its entry fence covers S
  ub12 = __builtin_amdgcn_readfirstlane(
      ged_induced(n1, n2, p, t1, m1, S.t[1], S.mask[1], S.phi, sumdeg, lane, f12));
  ged_lsap(n2, n1, 1, S.t[1], S.deg[1], t1, d1, S.u, lane, p);
  ub21 = __builtin_amdgcn_readfirstlane(
      ged_induced(n2, n1, p, t2, m2, S.t[0], S.mask[0], S.phi, sumdeg, lane, f21));
  lb0 = __builtin_amdgcn_readfirstlane(
      (ged_lsap(n1, n2, 2, S.t[0], S.deg[0], t2, d2, S.u, lane, p) + 1) >> 1);
}

// The search of a loaded pair (X.bp holds it, fenced) with max(n1, n2) <= 16 from the
// incumbent cost `inc`, at most `budget` > 0 expansions.  A complete map cheaper than the
// incumbent replaces it: inc is its cost and best the graph-1 node of this lane's graph-2 node.
// Returns whether the root's children ended before the budget did; nexp is the expansions
// spent.
__device__ __forceinline__ bool ged_search(GedExactLds &X, const int n1, const int n2,
                                           const int lane, const uint32_t m1, const int t1,
                                           const uint32_t m2, const int t2, const int64_t budget,
                                           int &inc, int &best, int64_t &nexp) {
  GedLds &S = X.bp;
  const int d2 = __popc(m2);
  bool ended = false;
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
  const int64_t steps = budget * (kExLanes + 3) + 4;   // an expansion, <= 17 children, a return
  for (int64_t it = 0; it < steps; ++it) {
    // the search state is the same in every lane: keep it in scalar registers
    k = __builtin_amdgcn_readfirstlane(k);
    g = __builtin_amdgcn_readfirstlane(g);
    I = __builtin_amdgcn_readfirstlane(I);
    EU = __builtin_amdgcn_readfirstlane(EU);
    inc = __builtin_amdgcn_readfirstlane(inc);
    expand = __builtin_amdgcn_readfirstlane(expand);
    if (expand) {
      if (nexp == budget) break;
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
        ended = true;
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
  return ended;
}

}  // namespace
