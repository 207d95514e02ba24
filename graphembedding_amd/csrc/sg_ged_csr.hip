// sg_ged_csr.hip — graph edit distance bounds for every pair of a query x database grid of a
// graph store (include/siamese_ged_csr.h): the bipartite approximation of Riesen & Bunke for
// graphs of up to 512 nodes, N = n1 + n2 <= 1024.  Two launches per call: the m + n entries'
// packed (type, degree) words into the workspace, then one wavefront per pair.
//
// Mapping.  Column c of the N x N assignment problem belongs to lane c & 63, slot c >> 6, so a
// lane owns up to 16 columns.  The grid kernel is instantiated for slot capacities S = 1, 2, 4,
// 8, 16 and the launch takes the smallest with 2 n_max <= 64 S (registers and LDS are sized by
// S); inside, every slot loop is unrolled over S and guarded by the wave-uniform s < ceil(N / 64),
// so a pair pays for its own N.  Per column v, the distance, `way`, the marked bit and the
// column's packed word are registers reached by static unrolling only; what a round reads at a
// dynamic column or row (p[j0], u[i0], the row's packed word, way[j0] on the way back) lives in
// the wavefront's LDS.  No barriers: the wavefronts of a workgroup share nothing.
//
// The solver keeps distances from the entering row instead of minv net of the deltas: a round's
// candidate is C[i0][c] - u[i0] - v[c] + dist(j0), compared on strict < with the column's best,
// and the potentials move once per row (v[c] -= T - dist[c], u[p[c]] += T - dist[c] for the
// marked columns, T the distance of the free column reached).  Both sides of every comparison
// are the header's minv plus the same sum of deltas, so rounds, ties and results are the
// header's; the bounds of its "Integer widths" hold for these distances as they do for minv
// (a candidate is at most F - v[c] + dist(j0) <= F + opt_(i+1) <= F + D).
//
// The dense units (sg_ged.hip, sg_ged_exact.hip, sg_ged_beam.hip, sg_ged_common.h) are not
// touched and nothing of theirs is included: their 64-lane solver does not carry over.
#include "../../include/siamese_ged_csr.h"
#include "sg_common.h"

namespace {

constexpr int kCsrGedMaxNodes = 512;                   // N = n1 + n2 <= 1024: 16 slots of 64
constexpr int64_t kCsrGedMaxSide = (int64_t)1 << 24;   // m, n
constexpr int64_t kCsrGedMaxPairs = (int64_t)1 << 32;  // m * n: one wavefront per pair
constexpr int kCsrGedWaves = 4;                        // wavefronts (pairs) per workgroup
constexpr int kCsrGedBig = 1 << 21;                    // forbidden entries (header: F)
constexpr int kCsrGedInf = 0x7FFFFFFF;                 // a column's distance before round one
constexpr int kCsrGedDegBits = 10;                     // packed word: type << 10 | degree
constexpr uint32_t kCsrGedDegMask = (1u << kCsrGedDegBits) - 1u;
constexpr int kCsrGedMaxType = 1 << 22;

// workspace entry of one q / db id, in 4-byte words: [n_max] packed (type, degree) words, the
// node count (-1 for an entry that cannot be served), the store graph id
__host__ __device__ inline int csr_ged_entry_words(int n_max) { return (n_max + 2 + 3) & ~3; }

struct CsrGedStore {
  const int32_t *node_off, *types, *row_ptr, *col;
  const float *val;
  int n_graphs, n_max;
};

struct CsrGedPrepArgs {
  CsrGedStore st;
  const int32_t *qidx, *dbidx;   // or null: entry k is graph k
  int64_t m, total;              // entries [0, m) are queries, [m, total) database graphs
  int32_t *ws;
  int32_t *status;
};

struct CsrGedGridArgs {
  CsrGedStore st;
  const int32_t *ws;
  int both;
  int64_t m, n, ld;
  int32_t *ub, *lb;   // lb or null
  int16_t *map;       // or null
};

// the wavefront's LDS at slot capacity S: both graphs' packed words by node, the row potentials,
// the row of every column, the way back by column and the assignment by row
template <int S>
struct CsrGedLds {
  uint32_t g[2][32 * S];
  int32_t u[64 * S];
  int16_t p[64 * S];
  int16_t way[64 * S];
  int16_t phi[32 * S];
};

__device__ __forceinline__ int csr_ged_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// minimum of a packed (distance << 10 | column) key over the wavefront, as a scalar
__device__ __forceinline__ uint32_t csr_ged_wave_min(uint32_t k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = __shfl_xor(k, o, 64);
    k = x < k ? x : k;
  }
  return __builtin_amdgcn_readfirstlane(k);
}

// ---------------------------------------------------------------------------
// One wavefront per q / db entry: lanes stride over the graph's nodes, each counting the
// off-diagonal non-zero entries of its CSR row, one entry after the other: up to 512 loads per
// lane for a dense graph, once per entry and call, next to up to 3 N^2 rounds per pair.
// The header's preconditions on the store (symmetric, columns strictly ascending inside [0, n))
// are the caller's and are not checked here: a store that breaks them gets wrong bounds without
// a status.  Nothing is read or written out of bounds then: the degree is clamped to the 10 bits
// it has, and the induced cost skips a column outside the graph.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kCsrGedWaves *SG_WAVE) sg_csr_ged_prep_kernel(CsrGedPrepArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t e = (int64_t)blockIdx.x * kCsrGedWaves + wave;
  if (e >= A.total) return;
  const bool isq = e < A.m;
  const int64_t k = isq ? e : e - A.m;
  const int32_t *idx = isq ? A.qidx : A.dbidx;
  const int64_t id = idx ? (int64_t)idx[k] : k;
  const bool in_store = id >= 0 && id < A.st.n_graphs;
  const int nm = A.st.n_max;
  const int off = in_store ? A.st.node_off[id] : 0;
  const int n = in_store ? A.st.node_off[id + 1] - off : 0;
  int32_t *dst = A.ws + e * csr_ged_entry_words(nm);
  bool ok = in_store && n >= 1 && n <= nm;
  if (ok) {
    bool bad = false;
    for (int a = lane; a < n; a += SG_WAVE) {
      const int t = A.st.types[off + a];
      const int s0 = A.st.row_ptr[off + a], s1 = A.st.row_ptr[off + a + 1];
      int deg = 0;
      for (int s = s0; s < s1; ++s) deg += (A.st.col[s] != a && A.st.val[s] != 0.f) ? 1 : 0;
      deg = deg < n ? deg : n - 1;   // strictly ascending columns inside [0, n) give no more
      bad = bad || t < 0 || t >= kCsrGedMaxType;
      dst[a] = (int32_t)(((uint32_t)t << kCsrGedDegBits) | (uint32_t)deg);
    }
    ok = __ballot(bad) == 0ull;
  }
  if (lane == 0) {
    if (!ok && A.status)
      atomicExch(A.status, (int32_t)(in_store ? SG_ERR_SHAPE : SG_ERR_ARG));
    dst[nm] = ok ? n : -1;
    dst[nm + 1] = ok ? (int32_t)id : -1;
  }
}

// ---------------------------------------------------------------------------
// The assignment problem of nr row nodes (packed words rg) against nc column nodes (cg),
// N = nr + nc <= 64 S, on the header's matrix with substitution weight w.  Returns the optimum
// Σu + Σv; L.p holds the row of every column.
// ---------------------------------------------------------------------------
template <int S>
__device__ __forceinline__ int csr_ged_lsap(const int nr, const int nc, const int w,
                                            const uint32_t *rg, const uint32_t *cg,
                                            CsrGedLds<S> &L, const int lane) {
  const int N = nr + nc;
  const int ns = (N + 63) >> 6;   // live slots, wave-uniform
  int v[S];
  uint32_t cw[S];
  uint32_t live = 0;              // bit s: column s * 64 + lane exists
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int c = s * 64 + lane;
    v[s] = 0;
    cw[s] = 0;
    if (c < N) {
      live |= 1u << s;
      // a real column's packed word; an epsilon column's own row (whose deletion it is)
      cw[s] = c < nc ? cg[c] : (uint32_t)(c - nc);
      L.u[c] = 0;
      L.p[c] = -1;
    }
  }
  sg_wsync();
  for (int i = 0; i < N; ++i) {
    int dist[S], way[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      dist[s] = kCsrGedInf;
      way[s] = -1;
    }
    uint32_t used = 0;      // bit s: this lane's column of slot s is marked
    int j0 = -1, i0 = i;    // the column marked last (-1: none yet) and its row
    int base = 0;           // dist(j0) - u[i0]
    int T = 0;              // the distance of the column marked last
    for (int r = 0; r < N; ++r) {
      uint32_t best = 0xFFFFFFFFu;
      const uint32_t open = live & ~used;
      if (i0 < nr) {   // a real row: substitutions, then its own deletion column
        const uint32_t rw = rg[i0];
        const uint32_t rd = rw & kCsrGedDegMask;
        const int del = w + (int)rd;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (s < ns) {
            const uint32_t x = cw[s];
            const int sub = (int)__sad(rd, x & kCsrGedDegMask,
                                       ((rw ^ x) >> kCsrGedDegBits) ? (uint32_t)w : 0u);
            const int eps = x == (uint32_t)i0 ? del : kCsrGedBig;
            const int cur = (lane < nc - s * 64 ? sub : eps) + base - v[s];
            if ((open >> s) & 1u) {
              if (cur < dist[s]) {
                dist[s] = cur;
                way[s] = j0;
              }
              const uint32_t key = ((uint32_t)dist[s] << 10) | (uint32_t)(s * 64 + lane);
              best = key < best ? key : best;
            }
          }
        }
      } else {         // an epsilon row: its own insertion column, then zeros
        const int own = i0 - nr;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (s < ns) {
            const int ins = own - s * 64 == lane ? w + (int)(cw[s] & kCsrGedDegMask) : kCsrGedBig;
            const int cur = (lane < nc - s * 64 ? ins : 0) + base - v[s];
            if ((open >> s) & 1u) {
              if (cur < dist[s]) {
                dist[s] = cur;
                way[s] = j0;
              }
              const uint32_t key = ((uint32_t)dist[s] << 10) | (uint32_t)(s * 64 + lane);
              best = key < best ? key : best;
            }
          }
        }
      }
      const uint32_t key = csr_ged_wave_min(best);
      if (key == 0xFFFFFFFFu) {   // no unmarked column: cannot happen while a row is unassigned
        j0 = -1;
        break;
      }
      j0 = (int)(key & 1023u);
      T = (int)(key >> 10);
      if (lane == (j0 & 63)) used |= 1u << (j0 >> 6);
      i0 = __builtin_amdgcn_readfirstlane((int)L.p[j0]);
      if (i0 < 0) break;   // a free column: the path ends
      base = T - __builtin_amdgcn_readfirstlane(L.u[i0]);
    }
    // the potentials of the marked columns and of their rows, once per row
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (s < ns) {
        const int c = s * 64 + lane;
        if ((used >> s) & 1u) {
          const int dd = T - dist[s];
          const int pc = L.p[c];
          v[s] -= dd;
          if (pc >= 0) L.u[pc] += dd;   // marked columns hold distinct rows
        }
        if ((live >> s) & 1u) L.way[c] = (int16_t)way[s];
      }
    }
    if (lane == 0) L.u[i] = T;
    sg_wsync();
    for (int r = 0; r < N && j0 >= 0; ++r) {   // flip the path back to row i
      const int j1 = __builtin_amdgcn_readfirstlane((int)L.way[j0]);
      const int pj = j1 < 0 ? i : __builtin_amdgcn_readfirstlane((int)L.p[j1 < 0 ? 0 : j1]);
      sg_wsync();
      if (lane == 0) L.p[j0] = (int16_t)pj;
      sg_wsync();
      j0 = j1;
    }
  }
  int sum = 0;
#pragma unroll
  for (int s = 0; s < S; ++s)
    if ((live >> s) & 1u) sum += L.u[s * 64 + lane] + v[s];
  return csr_ged_wave_sum(sum);
}

// The cost of the edit path of the assignment in L.p, rows = store graph gr (nr nodes, packed
// words rg), columns = store graph gc.  sumdeg = 2 (|E1| + |E2|).  Leaves phi in L.phi: the
// column node of every row node, or -1.  Lanes stride over the row graph's CSR entries (a, b):
// a by bisection of row_ptr, then phi(b) by bisection of row phi(a) of the column graph; the
// store is symmetric, so every kept edge is counted from both ends.
template <int S>
__device__ __forceinline__ int csr_ged_induced(const CsrGedStore &st, const int nr, const int nc,
                                               const int gr, const int gc, const uint32_t *rg,
                                               const uint32_t *cg, CsrGedLds<S> &L,
                                               const int sumdeg, const int lane) {
  for (int a = lane; a < nr; a += SG_WAVE) L.phi[a] = -1;
  sg_wsync();
  for (int c = lane; c < nc; c += SG_WAVE) {
    const int r = L.p[c];
    if (r >= 0 && r < nr) L.phi[r] = (int16_t)c;
  }
  sg_wsync();
  int dels = 0, local = 0;
  for (int a = lane; a < nr; a += SG_WAVE) {
    const int f = L.phi[a];
    if (f < 0)
      ++dels;
    else
      local += ((rg[a] ^ cg[f]) >> kCsrGedDegBits) ? 1 : 0;
  }
  const int32_t *__restrict__ rp_r = st.row_ptr + st.node_off[gr];
  const int32_t *__restrict__ rp_c = st.row_ptr + st.node_off[gc];
  const int e0 = rp_r[0], e1 = rp_r[nr];
  for (int e = e0 + lane; e < e1; e += SG_WAVE) {
    const int b = st.col[e];
    if (st.val[e] == 0.f || (unsigned)b >= (unsigned)nr) continue;
    int lo = 0, hi = nr - 1;   // the largest a with row_ptr[a] <= e
    for (int k = 0; k < 10; ++k) {
      if (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rp_r[mid] <= e)
          lo = mid;
        else
          hi = mid - 1;
      }
    }
    const int a = lo;
    if (a == b) continue;
    const int fa = L.phi[a], fb = L.phi[b];
    if (fa < 0 || fb < 0) continue;
    const int s1 = rp_c[fa + 1];
    int l2 = rp_c[fa], h2 = s1;   // the first entry of row fa with column >= fb
    for (int k = 0; k < 10; ++k) {
      if (l2 < h2) {
        const int mid = (l2 + h2) >> 1;
        if (st.col[mid] < fb)
          l2 = mid + 1;
        else
          h2 = mid;
      }
    }
    if (l2 < s1 && st.col[l2] == fb && st.val[l2] != 0.f) --local;
  }
  const int d = csr_ged_wave_sum(dels);
  const int s = csr_ged_wave_sum(local);
  return d + (nc - nr + d) + s + sumdeg / 2;
}

// ---------------------------------------------------------------------------
// One wavefront per pair (i, j) of the grid.
// ---------------------------------------------------------------------------
template <int S>
__global__ void __launch_bounds__(kCsrGedWaves *SG_WAVE) sg_csr_ged_grid_kernel(CsrGedGridArgs A) {
  __shared__ CsrGedLds<S> lds[kCsrGedWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t pair = (int64_t)blockIdx.x * kCsrGedWaves + wave;
  if (pair >= A.m * A.n) return;
  const int64_t qi = pair / A.n, dj = pair - qi * A.n;
  const int nm = A.st.n_max, W = csr_ged_entry_words(nm);
  const int32_t *__restrict__ e1 = A.ws + qi * W;
  const int32_t *__restrict__ e2 = A.ws + (A.m + dj) * W;
  const int n1 = e1[nm], n2 = e2[nm];
  const int g1 = e1[nm + 1], g2 = e2[nm + 1];
  const int64_t o = qi * A.ld + dj;
  int16_t *map = A.map ? A.map + pair * nm : nullptr;
  if (n1 < 1 || n2 < 1 || n1 > 32 * S || n2 > 32 * S) {   // an entry the call cannot serve
    if (lane == 0) {
      A.ub[o] = -1;
      if (A.lb) A.lb[o] = -1;
    }
    if (map)
      for (int a = lane; a < nm; a += SG_WAVE) map[a] = -1;
    return;
  }
  CsrGedLds<S> &L = lds[wave];
  int sumdeg = 0;
  for (int a = lane; a < n1; a += SG_WAVE) {
    const uint32_t x = (uint32_t)e1[a];
    L.g[0][a] = x;
    sumdeg += (int)(x & kCsrGedDegMask);
  }
  for (int b = lane; b < n2; b += SG_WAVE) {
    const uint32_t x = (uint32_t)e2[b];
    L.g[1][b] = x;
    sumdeg += (int)(x & kCsrGedDegMask);
  }
  sumdeg = csr_ged_wave_sum(sumdeg);
  sg_wsync();
  // one solver body for the three problems: 1->2 and 2->1 at w = 1 with their induced costs,
  // then 1->2 at w = 2
  int ub = 0;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1 && !A.both) continue;
    if (pass == 2 && !A.lb) break;
    const bool swap = pass == 1;
    const int nr = swap ? n2 : n1, nc = swap ? n1 : n2;
    const uint32_t *rg = L.g[swap ? 1 : 0], *cg = L.g[swap ? 0 : 1];
    const int opt = csr_ged_lsap<S>(nr, nc, pass == 2 ? 2 : 1, rg, cg, L, lane);
    if (pass == 2) {
      if (lane == 0) A.lb[o] = (opt + 1) >> 1;
      break;
    }
    const int x = csr_ged_induced<S>(A.st, nr, nc, swap ? g2 : g1, swap ? g1 : g2, rg, cg, L,
                                     sumdeg, lane);
    if (pass == 0) {
      ub = x;
      if (map)
        for (int a = lane; a < nm; a += SG_WAVE) map[a] = a < n1 ? L.phi[a] : (int16_t)-1;
    } else {
      ub = x < ub ? x : ub;
    }
    sg_wsync();   // phi is rewritten by the next order
  }
  if (lane == 0) A.ub[o] = ub;
}

// the rules on m, n and n_max alone (siamese_ged_csr.h, in its order)
inline int csr_ged_shape_rc(int64_t m, int64_t n, int32_t n_max) {
  if (m < 0 || n < 0) return SG_ERR_ARG;
  if (n_max < 1) return SG_ERR_ARG;
  if (n_max > kCsrGedMaxNodes) return SG_ERR_UNSUPPORTED;
  if (m > kCsrGedMaxSide || n > kCsrGedMaxSide || m * n > kCsrGedMaxPairs)
    return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

template <int S>
void csr_ged_launch_grid(const CsrGedGridArgs &G, hipStream_t stream) {
  hipLaunchKernelGGL(sg_csr_ged_grid_kernel<S>,
                     dim3((unsigned)((G.m * G.n + kCsrGedWaves - 1) / kCsrGedWaves)),
                     dim3(kCsrGedWaves * SG_WAVE), 0, stream, G);
}

}  // namespace

extern "C" {

int64_t sg_csr_ged_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max) {
  if (csr_ged_shape_rc(m, n, n_max) != SG_OK) return -1;
  if (m == 0 || n == 0) return 0;
  return (m + n) * (int64_t)csr_ged_entry_words(n_max) * 4;
}

int32_t sg_csr_ged_grid(const sg_csr_store_t *store, const int32_t *q_idx, int64_t m,
                        const int32_t *db_idx, int64_t n, int32_t both_orders,
                        int32_t *ub_out, int64_t ld, int32_t *lb_out, int16_t *map_out,
                        int32_t *status_out, void *workspace, sg_stream_t stream) {
  if (m < 0 || n < 0 || ld < 0) return SG_ERR_ARG;
  if (store && store->n_graphs < 0) return SG_ERR_ARG;
  // a NULL store has no n_max: the rules on m and n alone, at a capacity they accept
  const int rc = csr_ged_shape_rc(m, n, store ? store->n_max : 1);
  if (rc != SG_OK) return rc;
  if (ld < n) return SG_ERR_ARG;
  if (both_orders != 0 && both_orders != 1) return SG_ERR_ARG;
  if (m == 0 || n == 0) return SG_OK;
  if (!store || !store->node_off || !store->types || !store->row_ptr || !store->col ||
      !store->val || !ub_out || !workspace)
    return SG_ERR_ARG;
  CsrGedStore st;
  st.node_off = store->node_off;
  st.types = store->types;
  st.row_ptr = store->row_ptr;
  st.col = store->col;
  st.val = store->val;
  st.n_graphs = store->n_graphs;
  st.n_max = store->n_max;
  CsrGedPrepArgs P;
  P.st = st;
  P.qidx = q_idx;
  P.dbidx = db_idx;
  P.m = m;
  P.total = m + n;
  P.ws = (int32_t *)workspace;
  P.status = status_out;
  hipLaunchKernelGGL(sg_csr_ged_prep_kernel,
                     dim3((unsigned)((m + n + kCsrGedWaves - 1) / kCsrGedWaves)),
                     dim3(kCsrGedWaves * SG_WAVE), 0, (hipStream_t)stream, P);
  CsrGedGridArgs G;
  G.st = st;
  G.ws = (const int32_t *)workspace;
  G.both = both_orders;
  G.m = m;
  G.n = n;
  G.ld = ld;
  G.ub = ub_out;
  G.lb = lb_out;
  G.map = map_out;
  const int slots = (2 * st.n_max + 63) / 64;   // the smallest capacity that holds 2 n_max
  if (slots <= 1)
    csr_ged_launch_grid<1>(G, (hipStream_t)stream);
  else if (slots <= 2)
    csr_ged_launch_grid<2>(G, (hipStream_t)stream);
  else if (slots <= 4)
    csr_ged_launch_grid<4>(G, (hipStream_t)stream);
  else if (slots <= 8)
    csr_ged_launch_grid<8>(G, (hipStream_t)stream);
  else
    csr_ged_launch_grid<16>(G, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
