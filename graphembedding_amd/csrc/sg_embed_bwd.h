// sg_embed_bwd.h — the fixed-order sum of per-workgroup partial rows, which both embed-once
// backwards end in: the node-stack backward (sg_embed_nodes.hip) sums its gradient slabs with
// it, the grid call (sg_embed_train.hip) the partials of gQ and g_emb_db.  Kept out of
// sg_embed_plan.h so that the units without a backward (sg_embed.hip, sg_search.hip) do not
// compile a kernel they never launch.
// Internal linkage: each unit compiles its own copy.
#pragma once
#include "sg_embed_plan.h"

namespace {

// dst[c] = Σ_r src[r][c], rows in order (deterministic)
__global__ void __launch_bounds__(256) sg_sum_rows(const float *__restrict__ src, int64_t rows,
                                                   int64_t cols, float *__restrict__ dst) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cols) return;
  float acc = 0.f;
  for (int64_t r = 0; r < rows; ++r) acc += src[r * cols + t];
  dst[t] = acc;
}

}  // namespace
