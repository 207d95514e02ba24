// sg_search_split.h — how a fused search call is cut, for the three units that have one
// (sg_search.hip: NTN head at D <= 31; sg_web_search.hip: graph-store models; sg_dot_grid.hip:
// Dot head): S segments of seg database columns times nqc chunks of qb queries, one workgroup
// each, and the candidate part of the workspace.  Everything here is a function of m, n, k,
// seg_cols and three numbers of the unit (SearchUnit); what depends on the model (its plan,
// the kernel's own LDS, the Q tables) stays with the unit.
// Plain C++: no HIP and no device code, so a host compiler builds it alone
// (tests/test_search_split_host.py).  Internal linkage: each unit compiles its own copy.
#pragma once
#include "../../include/siamese_hip.h"

namespace {

constexpr int kTopkMax = 64;            // one list entry per lane
constexpr int kListBytes = 12;          // a list entry: 64-bit key + the value's bits
constexpr int64_t kSegMin = 1024;       // the library's own segment choice lies in [kSegMin,
                                        // 65536] columns: 1024 per list entry, and k <= 64
constexpr int64_t kSearchMaxRows = (int64_t)1 << 29;   // kMaxRows (sg_embed_plan.h), which
                                                       // sg_search_lists.h asserts

// What differs between the units
struct SearchUnit {
  int64_t target;   // workgroups that fill the device: sg_num_cus() times 8, or 2 (Web)
  int granule;      // queries a chunk is a multiple of: 4, or 16 (Dot)
  int list_lds;     // LDS bytes for the lists of a workgroup's queries
};

struct SearchSplit {
  int64_t seg, nseg, nqc, qb, blocks;
  int64_t cand;         // candidate entries, nseg · m · k
  int64_t cand_bytes;   // their part of the workspace
};

// Every host check on k, seg_cols, m and n, in sg_topk_rows' order, then seg_cols, then the
// row limits; then the cut.  m >= 0 and n >= 0 are the caller's, with its model plan.
inline int search_split(const SearchUnit &u, int64_t m, int64_t n, int32_t k, int64_t seg_cols,
                        SearchSplit *S) {
  if (k < 1) return SG_ERR_ARG;
  if (k > kTopkMax) return SG_ERR_UNSUPPORTED;
  if (k > n) return SG_ERR_ARG;
  if (seg_cols < 0 || (seg_cols & 63) != 0) return SG_ERR_ARG;
  if (m > kSearchMaxRows || n > kSearchMaxRows) return SG_ERR_UNSUPPORTED;   // n < 2^31 with it
  const int64_t gr = u.granule;
  const int64_t max_qc = m > gr ? (m + gr - 1) / gr : 1;
  int64_t seg = seg_cols;
  if (seg == 0) {
    // a list costs about k (1 + ln(seg / k)) insertions per segment and k rounds over
    // its k candidates in the merge: segments of 1024 columns per list entry (at least
    // 4096) amortise both, shorter ones only where the queries alone cannot fill the device
    seg = 4096;
    while (seg < 1024 * (int64_t)k) seg <<= 1;   // k <= 64: at most 65536
    while (seg > kSegMin && ((n + seg - 1) / seg) * max_qc < u.target) seg >>= 1;
  }
  if (seg > n) seg = (n + 63) & ~(int64_t)63;   // one segment (k <= n: n >= 1)
  S->seg = seg;
  S->nseg = (n + seg - 1) / seg;
  // query chunks as grid_split cuts them: enough to reach the target, else as many
  // queries as possible per load of the database tiles, within the LDS of the lists
  int64_t nqc = (u.target + S->nseg - 1) / S->nseg;
  nqc = nqc > max_qc ? max_qc : nqc;
  int64_t qb = (((m + nqc - 1) / nqc) + gr - 1) & ~(gr - 1);
  // lowest at k = 64: 40 of 32768 B at granule 4, 32 at granule 16, 16 of 12288 B
  const int64_t qb_cap = (u.list_lds / (kListBytes * k)) & ~(gr - 1);
  qb = qb > qb_cap ? qb_cap : qb;
  qb = qb < gr ? gr : qb;
  S->qb = qb;
  S->nqc = m > 0 ? (m + qb - 1) / qb : 1;
  S->blocks = S->nseg * S->nqc;
  if (S->blocks > 0x7FFFFFFF) return SG_ERR_UNSUPPORTED;
  S->cand = S->nseg * m * k;
  // the library's own choice depends on m and on the device: its workspace is sized for
  // the shortest segments it may pick, so the size is monotone and the same everywhere
  const int64_t ws_seg = seg_cols == 0 ? (n + kSegMin - 1) / kSegMin : S->nseg;
  S->cand_bytes = ws_seg * m * k * kListBytes + 256;
  return SG_OK;
}

}  // namespace
