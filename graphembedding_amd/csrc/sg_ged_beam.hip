// sg_ged_beam.hip — beam-search graph edit distance for every pair of a query x database grid
// (include/siamese_ged_beam.h): a level-synchronous beam of at most `width` states over node
// maps, seeded with the bipartite bounds of sg_ged_common.h.  Two launches per call: the m + n
// entries' adjacency bit masks into the workspace (sg_ged.hip's), then one wavefront per pair.
//
// Lane mapping of an expansion: lane j < n2 is graph-2 node j, lane n2 is epsilon, so the step
// cost, h and f of all n2 + 1 <= 33 children of a state are computed at once, each in its lane,
// against the parent's `used` mask and the images of node k's mapped neighbours (one ballot over
// the parent's map).  A state lives in LDS, double-buffered by level: its map by graph-2 node
// (psi: the graph-1 node mapped to node j, or -1; 32 bytes), `used`, and g, the running type
// intersection I and the used-edge count EU packed in one word.
//
// Selection: every child's f (or kBeamNone where it is pruned) is materialised as 16 bits at
// index p * (n2 + 1) + j, which is the (parent slot, graph-2 index, epsilon last) order.  The
// level's survivors are then taken in ascending f, one distinct f value per pass: a pass ranks
// the candidates of that f in index order by ballots and prefix popcounts (a stable counting
// sort) and finds the next f present, so the first `width` keys come out in order without a
// sort and without the f values nobody holds.  The chosen (p, j) are rebuilt into child states
// by one lane each.  All loop-controlling values (level, state count, pass, chunk) are
// wave-uniform.
#include "../../include/siamese_ged_beam.h"
#include "sg_ged_common.h"

namespace {

constexpr int kBeamMaxWidth = 128;
constexpr int kBeamLanes = kGedMaxNodes + 1;   // children of a state: n2 nodes + epsilon
constexpr int kBeamNone = 0xFFFF;              // a pruned child: above every f
constexpr int64_t kBeamGridX = (int64_t)1 << 20;   // pairs per grid row: 2^32 pairs in 2^12 rows
constexpr int kBeamIdxBits = 13;               // candidate indices < 128 * 33 = 4224 < 2^13

struct GedBeamArgs {
  const int32_t *ws;
  int n_max, width;
  int64_t m, n, ld;
  int32_t *ub, *lb;
  int8_t *map;    // or null
  int32_t *exp;   // or null
};

// the wavefront's LDS: the seed's, the two levels' states, the level's candidates and choice,
// and per graph-1 node k / graph-2 node j the masks of the nodes of its type on both sides,
// and the edges of E1 with an end above k
struct GedBeamLds {
  GedLds bp;
  uint32_t psi[2][kBeamMaxWidth][kGedMaxNodes / 4];
  uint32_t used[2][kBeamMaxWidth];
  uint32_t st[2][kBeamMaxWidth];   // g | I << 16 | EU << 22
  uint32_t img[kBeamMaxWidth];     // of the level's states: the images of node k's neighbours
  uint16_t cand[kBeamMaxWidth * kBeamLanes];
  uint16_t sel[kBeamMaxWidth];
  uint32_t T1[kGedMaxNodes], T2[kGedMaxNodes], K1[kGedMaxNodes], K2[kGedMaxNodes];
  int32_t pd[kGedMaxNodes], e1r[kGedMaxNodes];
};

// what is the same for every child of level k
struct GedBeamLevel {
  int k, nb, t1k, c1k, e1rk, r1;
  uint32_t m1k, T2k, notk;
};

// the child of a state (used, img, g, I, EU) that maps node k to graph-2 node j (sub: t2j, m2j
// its type and row mask, K1j / K2j the nodes of its type) or to epsilon: siamese_ged_exact.h's
// step cost and h
__device__ __forceinline__ void ged_beam_child(const GedBeamLevel &L, const int n2, const int E2,
                                               const uint32_t used, const uint32_t img,
                                               const int g, const int I, const int EU,
                                               const bool sub, const int t2j, const uint32_t m2j,
                                               const uint32_t K1j, const uint32_t K2j, int &gc,
                                               int &Ic, int &EUc, int &h) {
  const int dele = L.nb - __popc(img);
  const int c = sub ? (L.t1k != t2j ? 1 : 0) + __popc(img ^ (m2j & used)) + dele : 1 + L.nb;
  const int Ik = I - (L.c1k <= __popc(L.T2k & ~used) ? 1 : 0);
  Ic = Ik - (sub && __popc(K2j & ~used) <= __popc(K1j & L.notk) ? 1 : 0);
  EUc = EU + (sub ? __popc(m2j & used) : 0);
  const int r2c = n2 - __popc(used) - (sub ? 1 : 0);
  h = (L.r1 > r2c ? L.r1 : r2c) - Ic + abs(L.e1rk - (E2 - EUc));
  gc = g + c;
}

__device__ __forceinline__ int ged_beam_psi(const uint32_t *psi, const int j) {
  return (int)(int8_t)(psi[(j & 31) >> 2] >> ((j & 3) * 8));
}

// ---------------------------------------------------------------------------
// One wavefront (one workgroup) per pair (i, j) of the grid.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(SG_WAVE) sg_ged_beam_kernel(GedBeamArgs A) {
  __shared__ GedBeamLds X;
  const int lane = threadIdx.x;
  const int64_t pair = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
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
  // the incumbent's map by graph-2 node: f21 is one already, f12 is turned round in LDS
  if (lane < kGedMaxNodes) S.phi[lane] = -1;
  sg_wsync();
  if (lane < n1 && f12 >= 0) S.phi[f12] = lane;
  sg_wsync();
  const int inv12 = lane < kGedMaxNodes ? S.phi[lane] : -1;
  sg_wsync();
  int best = ub21 < ub12 ? f21 : inv12;
  int inc = ub21 < ub12 ? ub21 : ub12;
  int nexp = 0;
  bool proven = lb0 == inc;

  if (!proven && A.width > 0) {
    const int width = A.width, stride = n2 + 1;
    // per graph-1 node the nodes of its type on both sides; per graph-2 node the same
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
    if (lane < kGedMaxNodes) {
      X.K1[lane] = K1;
      X.K2[lane] = K2;
      X.pd[lane] = lane < n1 ? __popc(m1 & below) : 0;
    }
    sg_wsync();
    int I = 0;   // |multiset intersection| of all types: each type at its first graph-1 node
    if (lane < n1) {
      int s = 0;
      for (int a = 0; a < n1; ++a) s += a > lane ? X.pd[a] : 0;
      X.e1r[lane] = s;
      const uint32_t own1 = X.T1[lane], own2 = X.T2[lane];
      if ((own1 & below) == 0) I = __popc(own1) < __popc(own2) ? __popc(own1) : __popc(own2);
    }
    I = __builtin_amdgcn_readfirstlane(ged_wave_sum(I));
    const int E2 = __builtin_amdgcn_readfirstlane(ged_wave_sum(d2)) >> 1;
    // level 0: the root alone
    if (lane < kGedMaxNodes / 4) X.psi[0][0][lane] = 0xFFFFFFFFu;
    if (lane == 0) {
      X.used[0][0] = 0;
      X.st[0][0] = (uint32_t)I << 16;
    }
    sg_wsync();

    const uint64_t lt = lane == 0 ? 0ull : ~0ull >> (64 - lane);   // the lanes below this one
    int ns = 1, cur = 0;
    uint32_t leaf = 0xFFFFFFFFu;   // f << kBeamIdxBits | index of the first complete map
    bool truncated = false;
    for (int k = 0; k < n1; ++k) {
      GedBeamLevel L;
      L.k = k;
      L.m1k = (uint32_t)__builtin_amdgcn_readfirstlane((int)S.mask[0][k]);
      const uint32_t low = (1u << k) - 1u;
      L.nb = __popc(L.m1k & low);
      L.t1k = __builtin_amdgcn_readfirstlane(S.t[0][k]);
      L.c1k = __popc((uint32_t)__builtin_amdgcn_readfirstlane((int)X.T1[k]) & ~low);
      L.T2k = (uint32_t)__builtin_amdgcn_readfirstlane((int)X.T2[k]);
      L.e1rk = __builtin_amdgcn_readfirstlane(X.e1r[k]);
      L.r1 = n1 - k - 1;
      L.notk = ~(low | (1u << k));
      // expand every state of the level: lane j holds child j's f
      int fmin = kBeamNone, alive = 0;
      for (int p = 0; p < ns; ++p) {
        const uint32_t used = (uint32_t)__builtin_amdgcn_readfirstlane((int)X.used[cur][p]);
        const uint32_t st = (uint32_t)__builtin_amdgcn_readfirstlane((int)X.st[cur][p]);
        const int ps = ged_beam_psi(X.psi[cur][p], lane);
        const uint32_t img =
            (uint32_t)__ballot(lane < n2 && ps >= 0 && ((L.m1k >> (ps & 31)) & 1u));
        if (lane == 0) X.img[p] = img;
        const bool sub = lane < n2 && !((used >> (lane & 31)) & 1u), eps = lane == n2;
        int gc, Ic, EUc, h;
        ged_beam_child(L, n2, E2, used, img, (int)(st & 0xFFFFu), (int)((st >> 16) & 63u),
                       (int)(st >> 22), sub, t2, m2, K1, K2, gc, Ic, EUc, h);
        const int f = gc + h;
        const bool ok = (sub || eps) && f < inc;
        if (lane <= n2) X.cand[p * stride + lane] = (uint16_t)(ok ? f : kBeamNone);
        alive += __popcll(__ballot(ok));
        fmin = ok && f < fmin ? f : fmin;
      }
      nexp += ns;
      sg_wsync();
      alive = __builtin_amdgcn_readfirstlane(alive);
      if (alive == 0) break;   // every child pruned: the search is complete
      const int nc = ns * stride;
      if (k == n1 - 1) {   // complete maps: the first in (f, p, j) is the result
        uint32_t key = 0xFFFFFFFFu;
        for (int c0 = 0; c0 < nc; c0 += SG_WAVE) {
          const int i = c0 + lane;
          const uint32_t fv = i < nc ? X.cand[i] : (uint32_t)kBeamNone;
          const uint32_t kv = fv == (uint32_t)kBeamNone ? 0xFFFFFFFFu
                                                        : (fv << kBeamIdxBits) | (uint32_t)i;
          key = kv < key ? kv : key;
        }
        leaf = ged_wave_min(key);
        break;
      }
      const int want = alive < width ? alive : width;
      truncated = truncated || alive > width;
      // the first `want` survivors in (f, index) order: one distinct f per pass
      uint32_t v = ged_wave_min((uint32_t)fmin);
      int base = 0;
      for (int pass = 0; pass < want; ++pass) {
        uint32_t next = kBeamNone;
        for (int c0 = 0; c0 < nc; c0 += SG_WAVE) {
          const int i = c0 + lane;
          const uint32_t fv = i < nc ? X.cand[i] : (uint32_t)kBeamNone;
          const bool hit = fv == v;
          const uint64_t b = __ballot(hit);
          const int pos = base + __popcll(b & lt);
          if (hit && pos < want) X.sel[pos] = (uint16_t)i;
          base += __popcll(b);
          next = fv > v && fv < next ? fv : next;
          if (base >= want) break;
        }
        if (base >= want) break;
        v = ged_wave_min(next);
      }
      sg_wsync();
      // each chosen (p, j) becomes a state of level k + 1, one lane each
      const int nxt = cur ^ 1;
      for (int c0 = 0; c0 < want; c0 += SG_WAVE) {
        const int pos = c0 + lane;
        if (pos < want) {
          const int idx = X.sel[pos];
          const int p = idx / stride, j = idx - p * stride;
          const bool sub = j < n2;
          const int jj = sub ? j : 0;
          const uint32_t used = X.used[cur][p], st = X.st[cur][p];
          int gc, Ic, EUc, h;
          ged_beam_child(L, n2, E2, used, X.img[p], (int)(st & 0xFFFFu), (int)((st >> 16) & 63u),
                         (int)(st >> 22), sub, S.t[1][jj], S.mask[1][jj], X.K1[jj], X.K2[jj], gc,
                         Ic, EUc, h);
          X.used[nxt][pos] = sub ? used | (1u << jj) : used;
          X.st[nxt][pos] = (uint32_t)gc | ((uint32_t)Ic << 16) | ((uint32_t)EUc << 22);
          const int sh = (jj & 3) * 8;
#pragma unroll
          for (int q = 0; q < kGedMaxNodes / 4; ++q) {
            uint32_t w = X.psi[cur][p][q];
            if (sub && (jj >> 2) == q) w = (w & ~(0xFFu << sh)) | ((uint32_t)k << sh);
            X.psi[nxt][pos][q] = w;
          }
        }
      }
      ns = want;
      cur = nxt;
      sg_wsync();
    }
    proven = !truncated;
    if (leaf != 0xFFFFFFFFu) {   // the map of the first complete one: its parent's plus node n1-1
      const int idx = (int)(leaf & ((1u << kBeamIdxBits) - 1u));
      const int p = idx / stride, j = idx - p * stride;
      inc = (int)(leaf >> kBeamIdxBits);
      best = lane < kGedMaxNodes ? ged_beam_psi(X.psi[cur][p], lane) : -1;
      if (lane == j && j < n2) best = n1 - 1;
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

int64_t sg_ged_beam_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max) {
  if (ged_shape_rc(m, n, n_max) != SG_OK) return -1;
  if (m == 0 || n == 0) return 0;
  return (m + n) * (int64_t)ged_entry_words(n_max) * 4;
}

int32_t sg_ged_beam_grid(const float *store_adj, const int32_t *store_types,
                         const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                         const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                         int32_t width, int32_t *ub_out, int64_t ld, int32_t *lb_out,
                         int8_t *map_out, int32_t *expanded_out, int32_t *status_out,
                         void *workspace, sg_stream_t stream) {
  if (m < 0 || n < 0 || ld < 0) return SG_ERR_ARG;
  if (n_graphs < 0) return SG_ERR_ARG;
  const int rc = ged_shape_rc(m, n, n_max);
  if (rc != SG_OK) return rc;
  if (ld < n) return SG_ERR_ARG;
  if (width < 0) return SG_ERR_ARG;
  if (width > kBeamMaxWidth) return SG_ERR_UNSUPPORTED;
  if (m == 0 || n == 0) return SG_OK;
  if (!store_adj || !store_types || !store_n || !ub_out || !lb_out || !workspace)
    return SG_ERR_ARG;
  ged_launch_prep(store_adj, store_types, store_n, n_graphs, n_max, q_idx, m, db_idx, n,
                  status_out, workspace, (hipStream_t)stream);
  GedBeamArgs G;
  G.ws = (const int32_t *)workspace;
  G.n_max = n_max;
  G.width = width;
  G.m = m;
  G.n = n;
  G.ld = ld;
  G.ub = ub_out;
  G.lb = lb_out;
  G.map = map_out;
  G.exp = expanded_out;
  const int64_t pairs = m * n, gx = pairs < kBeamGridX ? pairs : kBeamGridX;
  hipLaunchKernelGGL(sg_ged_beam_kernel, dim3((unsigned)gx, (unsigned)((pairs + gx - 1) / gx)),
                     dim3(SG_WAVE), 0, (hipStream_t)stream, G);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
