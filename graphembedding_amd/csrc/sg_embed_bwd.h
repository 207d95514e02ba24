// sg_embed_bwd.h — what the two translation units with a node-stack backward share
// (sg_embed_train.hip: sg_embed_bwd_kernel; sg_embed_drop.hip: sg_embed_drop_bwd_kernel): the
// range of the gradient the kernels write, their launch shape, and the fixed-order sum of
// their per-workgroup slabs (which the grid call of sg_embed_train.hip uses for its partials
// as well).  Kept out of sg_embed_plan.h so that the units without a backward (sg_embed.hip,
// sg_search.hip) do not compile a kernel they never launch.
// Internal linkage throughout: each unit compiles its own copy.
#pragma once
#include "sg_embed_plan.h"

namespace {

// flat offset of the head's first variable: the node layers' range is [0, head_offset)
int head_offset(const SgGenPlan &P) { return P.head_kind == SG_NTN ? P.offW : P.n_params; }

// the generic kernel's backward shape with the node layers' gradient as the accumulator and
// one unit per two graphs; the workspace is one slab row per workgroup of this shape
SgGenLaunch embed_bwd_launch(const SgGenPlan &P, int64_t count) {
  return sg_gen_launch_shape(P, head_offset(P), (count + 1) / 2);
}

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
