// sg_search_lists.h — what the fused search kernels share (sg_search.hip: search at
// D <= 31, include/siamese_search.h; sg_web_search.hip: search for graph-store models at D in
// [32, 512], include/siamese_web_search.h; sg_dot_grid.hip: search for the Dot head,
// include/siamese_dot_embed.h): the running top-k list of one query, where a kernel leaves
// its lists, and the kernel that merges the candidate lists of a query's segments.  How a
// call is cut is sg_search_split.h; the key of the total order is topk_key
// (sg_embed_plan.h).  Internal linkage: each unit compiles its own copy.
#pragma once
#include "sg_embed_plan.h"
#include "sg_search_split.h"

namespace {

static_assert(kSearchMaxRows == kMaxRows, "the search's row limit is the grid's");

// ---------------------------------------------------------------------------
// The running top-k of one query: k keys in ascending order (best first) with the value
// bits beside them (a key does not keep the sign of a zero or a NaN's payload, and the
// two-call path returns the stored float).  Between column blocks a list rests in the
// wavefront's LDS; only its last key, the threshold, is read per block.  When a block has
// keys below the threshold the list is taken into registers, lane r the r-th entry (lanes
// >= k the all-ones sentinel), and the hits are inserted by rank in ascending lane order,
// a wave-uniform loop:  pos = popcount(ballot(entry < new)), lanes above pos take their
// lower neighbour's entry, lane pos takes the new one.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void list_insert(uint64_t *lk, float *lv, int k, int lane,
                                            uint64_t key, float s, uint64_t hits,
                                            uint64_t thr) {
  uint64_t mk = lane < k ? lk[lane] : ~0ull;
  float mv = lane < k ? lv[lane] : 0.f;
  while (hits) {
    const int src = __builtin_ctzll(hits);
    hits &= hits - 1;
    const uint64_t nk = readlane64(key, src);
    if (nk >= thr) continue;   // an earlier hit of this block lowered the threshold past it
    const float nv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), src));
    const int pos = __popcll(__ballot(mk < nk));   // < k: nk is below entry k - 1
    const uint64_t uk = __shfl_up(mk, 1, 64);
    const float uv = __shfl_up(mv, 1, 64);
    if (lane > pos) {
      mk = uk;
      mv = uv;
    }
    if (lane == pos) {
      mk = nk;
      mv = nv;
    }
    if (lane >= k) mk = ~0ull;   // what falls off the list
    thr = readlane64(mk, k - 1);
  }
  if (lane < k) {
    lk[lane] = mk;
    lv[lane] = mv;
  }
}

// An empty list: every key the all-ones sentinel
__device__ __forceinline__ void list_reset(uint64_t *lk, int k, int lane) {
  if (lane < k) lk[lane] = ~0ull;
}

// Lane l offers (key, s) to the list whose threshold thr = lk[k - 1] the caller has read
__device__ __forceinline__ void list_offer(uint64_t *lk, float *lv, int k, int lane,
                                           uint64_t key, float s, uint64_t thr) {
  const uint64_t hits = __ballot(key < thr);
  if (hits) {
    list_insert(lk, lv, k, lane, key, s, hits, thr);
    sg_wsync();
  }
}

// Where a search kernel leaves its lists; every *SearchArgs struct embeds one
struct ListOut {
  uint64_t *ckey;   // candidates [nseg][m][k], or
  float *cval;
  int32_t *idx;     // with one segment the results themselves [m][k]
  float *val;       // (may be null)
};

// ---------------------------------------------------------------------------
// Merge: one wavefront per query picks the k smallest of its nseg · k candidate keys by
// sg_topk_kernel's selection rounds (keys of distinct columns differ, so "the smallest key
// above the previous round's" is exact; the sentinels of a short segment are above every
// key and k <= n candidates are real).  The lane that held a round's winner writes it.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) sg_search_merge_kernel(const uint64_t *__restrict__ ckey,
                                                             const float *__restrict__ cval,
                                                             int64_t m, int nseg, int k,
                                                             int32_t *__restrict__ idx,
                                                             float *__restrict__ val) {
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  const uint32_t total = (uint32_t)nseg * (uint32_t)k;   // <= 2^23 segments · 64
  uint64_t prev = 0;   // below every key
  for (int r = 0; r < k; ++r) {
    uint64_t best = ~0ull;
    int64_t bpos = 0;
    for (uint32_t t = lane; t < total; t += SG_WAVE) {
      const uint32_t sgm = t / (uint32_t)k, e = t - sgm * (uint32_t)k;
      const int64_t pos = ((int64_t)sgm * m + i) * k + e;
      const uint64_t key = ckey[pos];
      if (key > prev && key < best) {
        best = key;
        bpos = pos;
      }
    }
    uint64_t win = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = __shfl_xor(win, o, 64);
      win = other < win ? other : win;
    }
    prev = win;
    if (best == win) {   // one lane: the keys are distinct
      idx[i * k + r] = (int32_t)(uint32_t)win;
      if (val) val[i * k + r] = cval[bpos];
    }
  }
}

// The candidate part of a workspace is [keys | values]
ListOut list_out(void *cand_ws, const SearchSplit &S, int32_t *idx_out, float *val_out) {
  ListOut O;
  O.ckey = (uint64_t *)cand_ws;
  O.cval = (float *)(O.ckey + S.cand);
  O.idx = idx_out;
  O.val = val_out;
  return O;
}

// The tail of every search call: with more than one segment the candidates are merged
void launch_search_merge(const ListOut &O, const SearchSplit &S, int64_t m, int32_t k,
                         hipStream_t st) {
  if (S.nseg > 1)
    hipLaunchKernelGGL(sg_search_merge_kernel, dim3((unsigned)m), dim3(64), 0, st, O.ckey,
                       O.cval, m, (int)S.nseg, (int)k, O.idx, O.val);
}

}  // namespace
