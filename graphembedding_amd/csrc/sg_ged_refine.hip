// sg_ged_refine.hip — 2-exchange refinement of the bipartite node maps for every pair of a query
// x database grid (include/siamese_ged_refine.h): steepest descent over the moves (a, x) "graph-1
// node a takes graph-2 node x, whoever held x takes a's old image", from both assignment orders'
// maps.  Two launches per call: the m + n entries' adjacency bit masks into the workspace
// (sg_ged.hip's), then one wavefront per pair, kGedWaves pairs per workgroup.
//
// There is no move to -1 alone: deleting a mapped node a and inserting its image adds a deletion
// and an insertion (2), saves at most the type mismatch (1) and loses 2 for every kept edge at
// a, so it changes the cost by 2 - mismatch + 2 (kept edges at a) >= 1 and never improves.
//
// State in LDS, per wavefront: both graphs' row masks and types (GedLds, the seed's), phi by
// graph-1 node, its inverse by graph-2 node, and per graph-1 node a the mask img[a] of its
// neighbours' images.  Every array has 32 dwords, so distinct entries lie on distinct banks.
//
// Lane mapping of a sweep: move c = a * n2 + x goes to lane c & 63 in round c >> 6 (a 32 x 32
// pair takes 16 rounds).  With y = phi[a] and b = inv[x] (-1 each: none), only the terms at a,
// b, x and y change:
//   mapped nodes   + 1 + [b, y both] - [y] - [b]          (each mapped node saves a deletion
//                                                          and an insertion)
//   mismatches     + mm(a, x) + [both] mm(b, y) - [y] mm(a, y) - [b] mm(b, x)
//   kept edges     + |img[a] & M2[x]| + [both] |img[b] & M2[y]|
//                  - [y] |img[a] & M2[y]| - [b] |img[b] & M2[x]|
//                  + 2 [both, a ~ b in graph 1, x ~ y in graph 2]
// The new terms leave the a-b edge out (bit x of img[a] meets the zero diagonal of M2[x], bit y
// of img[b] that of M2[y]) and the old terms count it at both ends, while it is kept before
// and after alike: hence the + 2.  The sweep's best move is one wave-wide minimum of
// cost << 10 | a << 5 | x (cost <= 64 + 2 * 496), which is the (cost, a, x) order.  All
// loop-controlling values (start, move, round) are wave-uniform.
#include "../../include/siamese_ged_refine.h"
#include "sg_ged_common.h"

namespace {

constexpr int kRefineMaxMoves = 4096;

struct GedRefineArgs {
  const int32_t *ws;
  int n_max, max_moves;
  int64_t m, n, ld;
  int32_t *ub, *lb;
  int8_t *map;      // or null
  int32_t *moves;   // or null
};

// the wavefront's LDS: the seed's, and the map being refined
struct GedRefineLds {
  GedLds bp;
  int32_t phi[kGedMaxNodes];    // by graph-1 node: its graph-2 node or -1
  int32_t inv[kGedMaxNodes];    // by graph-2 node: its graph-1 node or -1
  uint32_t img[kGedMaxNodes];   // by graph-1 node: the images of its neighbours
};

// ---------------------------------------------------------------------------
// One wavefront per pair (i, j) of the grid.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kGedWaves *SG_WAVE) sg_ged_refine_kernel(GedRefineArgs A) {
  __shared__ GedRefineLds lds[kGedWaves];
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
      if (A.moves) A.moves[o] = -1;
    }
    if (map && lane < nm) map[lane] = -1;
    return;
  }
  GedRefineLds &X = lds[wave];
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
  // the seed: both assignment orders and the lower bound, as sg_ged_exact_grid computes them
  int p0, f12, f21;
  ged_lsap(n1, n2, 1, S.t[0], S.deg[0], t2, d2, S.u, lane, p0);   // its entry fence covers S
  const int ub12 = __builtin_amdgcn_readfirstlane(
      ged_induced(n1, n2, p0, t1, m1, S.t[1], S.mask[1], S.phi, sumdeg, lane, f12));
  ged_lsap(n2, n1, 1, S.t[1], S.deg[1], t1, d1, S.u, lane, p0);
  const int ub21 = __builtin_amdgcn_readfirstlane(
      ged_induced(n2, n1, p0, t2, m2, S.t[0], S.mask[0], S.phi, sumdeg, lane, f21));
  const int lb0 = __builtin_amdgcn_readfirstlane(
      (ged_lsap(n1, n2, 2, S.t[0], S.deg[0], t2, d2, S.u, lane, p0) + 1) >> 1);
  const bool skipped = lb0 == (ub21 < ub12 ? ub21 : ub12);
  const int limit = skipped ? 0 : A.max_moves;
  const int nmoves = n1 * n2, rounds = (nmoves + SG_WAVE - 1) / SG_WAVE;
  // lane's move of round 0 and the step to the next round's: 64 = qa * n2 + rx
  const int a0 = lane / n2, x0 = lane - a0 * n2, qa = SG_WAVE / n2, rx = SG_WAVE - qa * n2;

  int best_phi = -1, best_cost = 0, accepted = 0;
  for (int start = 0; start < 2; ++start) {
    // the start's map by graph-1 node (f12 is one; f21 is the inverse of one) and its inverse
    if (lane < kGedMaxNodes) {
      X.phi[lane] = -1;
      X.inv[lane] = -1;
    }
    sg_wsync();
    if (start == 0) {
      if (lane < n1) X.phi[lane] = f12;
      if (lane < n1 && f12 >= 0) X.inv[f12] = lane;
    } else {
      if (lane < n2) X.inv[lane] = f21;
      if (lane < n2 && f21 >= 0) X.phi[f21] = lane;
    }
    sg_wsync();
    uint32_t img = 0;
    for (int b = 0; b < n1; ++b) {
      const int fb = X.phi[b];
      if (fb >= 0 && ((m1 >> b) & 1u)) img |= 1u << fb;
    }
    if (lane < kGedMaxNodes) X.img[lane] = img;
    sg_wsync();
    int cost = start == 0 ? ub12 : ub21;
    for (int mv = 0; mv < limit; ++mv) {
      uint32_t key = 0xFFFFFFFFu;
      int a = a0, x = x0;
      for (int r = 0; r < rounds; ++r) {
        if (r * SG_WAVE + lane < nmoves) {   // a < n1 and x < n2
          const int y = X.phi[a], b = X.inv[x];
          if (x != y) {
            const bool ym = y >= 0, bm = b >= 0, both = ym && bm;
            const int yy = y & 31, bb = b & 31;
            const uint32_t ia = X.img[a], ib = X.img[bb];
            const uint32_t M2x = S.mask[1][x], M2y = S.mask[1][yy];
            const int ta = S.t[0][a], tb = S.t[0][bb], tx = S.t[1][x], ty = S.t[1][yy];
            int dn = 1, ds = ta != tx ? 1 : 0, dk = __popc(ia & M2x);
            if (ym) {
              dn -= 1;
              ds -= ta != ty ? 1 : 0;
              dk -= __popc(ia & M2y);
            }
            if (bm) {
              dn -= 1;
              ds -= tb != tx ? 1 : 0;
              dk -= __popc(ib & M2x);
            }
            if (both) {
              dn += 1;
              ds += tb != ty ? 1 : 0;
              dk += __popc(ib & M2y);
              if (((S.mask[0][a] >> bb) & 1u) && ((M2x >> yy) & 1u)) dk += 2;
            }
            const int c = cost - 2 * dn + ds - 2 * dk;
            const uint32_t k = ((uint32_t)c << 10) | ((uint32_t)a << 5) | (uint32_t)x;
            key = k < key ? k : key;
          }
        }
        a += qa;
        x += rx;
        if (x >= n2) {
          x -= n2;
          a += 1;
        }
      }
      key = ged_wave_min(key);
      const int c = (int)(key >> 10);
      if (c >= cost) break;   // a local optimum (no legal move: the key is above every cost)
      // accept: a takes x, b = inv[x] takes y = phi[a]
      const int ma = (int)((key >> 5) & 31u), mx = (int)(key & 31u);
      const int my = __builtin_amdgcn_readfirstlane(X.phi[ma]);
      const int mb = __builtin_amdgcn_readfirstlane(X.inv[mx]);
      sg_wsync();
      if (lane < n1) {   // lane c's neighbours a and b have new images
        const bool na = (m1 >> ma) & 1u, nb = mb >= 0 && ((m1 >> (mb & 31)) & 1u);
        uint32_t v = X.img[lane];
        if (na && my >= 0) v &= ~(1u << (my & 31));
        if (nb) v &= ~(1u << mx);
        if (na) v |= 1u << mx;
        if (nb && my >= 0) v |= 1u << (my & 31);
        X.img[lane] = v;
      }
      if (lane == 0) {
        X.phi[ma] = mx;
        X.inv[mx] = ma;
        if (mb >= 0) X.phi[mb] = my;
        if (my >= 0) X.inv[my] = mb;
      }
      sg_wsync();
      cost = c;
      ++accepted;
    }
    const int f = lane < n1 ? X.phi[lane & 31] : -1;
    if (start == 0 || cost < best_cost) {
      best_cost = cost;
      best_phi = f;
    }
    sg_wsync();   // phi is rewritten by the next start
  }

  if (lane == 0) {
    A.ub[o] = best_cost;
    A.lb[o] = lb0;   // ub where they are equal: the descent proves nothing by itself
    if (A.moves) A.moves[o] = accepted;
  }
  if (map && lane < nm) map[lane] = (int8_t)best_phi;
}

}  // namespace

extern "C" {

int64_t sg_ged_refine_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max) {
  if (ged_shape_rc(m, n, n_max) != SG_OK) return -1;
  if (m == 0 || n == 0) return 0;
  return (m + n) * (int64_t)ged_entry_words(n_max) * 4;
}

int32_t sg_ged_refine_grid(const float *store_adj, const int32_t *store_types,
                           const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                           const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                           int32_t max_moves, int32_t *ub_out, int64_t ld, int32_t *lb_out,
                           int8_t *map_out, int32_t *moves_out, int32_t *status_out,
                           void *workspace, sg_stream_t stream) {
  if (m < 0 || n < 0 || ld < 0) return SG_ERR_ARG;
  if (n_graphs < 0) return SG_ERR_ARG;
  const int rc = ged_shape_rc(m, n, n_max);
  if (rc != SG_OK) return rc;
  if (ld < n) return SG_ERR_ARG;
  if (max_moves < 0) return SG_ERR_ARG;
  if (max_moves > kRefineMaxMoves) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !ub_out || !lb_out || !workspace)
    return SG_ERR_ARG;
  ged_launch_prep(store_adj, store_types, store_n, n_graphs, n_max, q_idx, m, db_idx, n,
                  status_out, workspace, (hipStream_t)stream);
  GedRefineArgs G;
  G.ws = (const int32_t *)workspace;
  G.n_max = n_max;
  G.max_moves = max_moves;
  G.m = m;
  G.n = n;
  G.ld = ld;
  G.ub = ub_out;
  G.lb = lb_out;
  G.map = map_out;
  G.moves = moves_out;
  hipLaunchKernelGGL(sg_ged_refine_kernel, dim3((unsigned)((m * n + kGedWaves - 1) / kGedWaves)),
                     dim3(kGedWaves * SG_WAVE), 0, (hipStream_t)stream, G);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
