// sg_eval.hip — device-side evaluation of the test matrix (include/siamese_eval.h): per query
// row the integer counts behind ap@k and MRR and the float64 squared-error sum behind "mse",
// from the float32 scores and the true tie-best ranks, without a sort.  The counts are what
// metrics.py derives from results.py's stable sorts, so they compare bit for bit.
#include "../../include/siamese_eval.h"
#include "sg_paths.h"

namespace {

constexpr int kEvalMaxK = 16;                       // k's per call
constexpr int64_t kEvalMaxCols = 32768;             // the row in LDS: 128 KB of the 160 KB
constexpr int64_t kEvalMaxRows = (int64_t)1 << 29;  // one workgroup per row
constexpr int kEvalThreads = 256;

struct EvalArgs {
  const float *scores;
  const int32_t *tr;
  const double *tsim;   // or null
  int64_t ld;
  int n, nk;
  int32_t ks[kEvalMaxK];
  int32_t *hits, *best, *nans;
  double *sqerr;        // null iff tsim is
};

__device__ __forceinline__ int eval_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------
// One workgroup of four wavefronts per query row.  The row is staged in LDS, padded to a
// multiple of 256 floats with NaN: both compares of the position rule are false against a
// NaN, so the padding (and the tail lanes of n % 64 != 0) never counts.
//   1. stage the row; per thread the NaN count, the maximum score over tr == 0 and the
//      strided float64 partial of the squared error (column tid, tid + 256, ... in order)
//   2. best = 1 + #{s' > that maximum}; the 256 partials fold in a fixed tree
//   3. the wavefronts take the candidates (tr < kmax) of every fourth 64-column chunk in
//      turn; a candidate's position p is popcount(ballot(better)) summed over the row on the
//      scalar side, four columns per lane per step (one 16-B LDS read).  p only grows, so the
//      walk ends once p reaches kmax: such a candidate is in no predicted top-k.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kEvalThreads) sg_eval_rows_kernel(EvalArgs A) {
  extern __shared__ __attribute__((aligned(16))) float row[];   // [np]
  __shared__ double sq[kEvalThreads];
  __shared__ float wmax[4];
  __shared__ int32_t ksl[kEvalMaxK];
  __shared__ int32_t cnt[2 + kEvalMaxK];   // NaNs, scores above the maximum, hits per k
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = A.n, np = (n + 255) & ~255, nk = A.nk;
  const int kmax = A.ks[nk - 1];
  const int64_t q = blockIdx.x;
  const float *__restrict__ s = A.scores + q * A.ld;
  const int32_t *__restrict__ tr = A.tr + q * (int64_t)n;
  const double *__restrict__ ts = A.tsim ? A.tsim + q * (int64_t)n : nullptr;
  if (tid < 2 + kEvalMaxK) cnt[tid] = 0;
  if (tid < kEvalMaxK) ksl[tid] = tid < nk ? A.ks[tid] : 0;
  float mx = -INFINITY;
  int nans = 0;
  double e = 0.0;
  for (int j = tid; j < np; j += kEvalThreads) {
    float v = __builtin_nanf("");
    if (j < n) {
      v = s[j];
      nans += v != v ? 1 : 0;
      if (tr[j] == 0 && v > mx) mx = v;
      if (ts) {
        const double d = ts[j] - (double)v;
        e += d * d;
      }
    }
    row[j] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  nans = eval_wave_sum(nans);
  if (lane == 0) wmax[wave] = mx;
  sq[tid] = e;
  __syncthreads();
  if (lane == 0 && nans) atomicAdd(&cnt[0], nans);
  mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  int above = 0;
  for (int i = 4 * tid; i < np; i += 4 * kEvalThreads) {
    const float4 v = *(const float4 *)(row + i);
    above += (v.x > mx ? 1 : 0) + (v.y > mx ? 1 : 0) + (v.z > mx ? 1 : 0) + (v.w > mx ? 1 : 0);
  }
  above = eval_wave_sum(above);
  if (lane == 0 && above) atomicAdd(&cnt[1], above);
  if (ts) {
    for (int h = kEvalThreads / 2; h > 0; h >>= 1) {
      if (tid < h) sq[tid] += sq[tid + h];
      __syncthreads();
    }
  }
  for (int j0 = 64 * wave; j0 < n; j0 += kEvalThreads) {
    const int j = j0 + lane;
    const int t = j < n ? tr[j] : 0x7FFFFFFF;
    uint64_t todo = __ballot(t < kmax);
    while (todo) {
      const int b = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int jc = j0 + b;
      const int tj = __shfl(t, b, 64);
      const float sj = row[jc];
      int p = 0;
      for (int i = 0; i < np && p < kmax; i += 256) {
        const int c = i + 4 * lane;
        const float4 v = *(const float4 *)(row + c);
        p += __popcll(__ballot(v.x > sj || (v.x == sj && c > jc)));
        p += __popcll(__ballot(v.y > sj || (v.y == sj && c + 1 > jc)));
        p += __popcll(__ballot(v.z > sj || (v.z == sj && c + 2 > jc)));
        p += __popcll(__ballot(v.w > sj || (v.w == sj && c + 3 > jc)));
      }
      if (lane < nk && tj < ksl[lane] && p < ksl[lane]) atomicAdd(&cnt[2 + lane], 1);
    }
  }
  __syncthreads();
  if (tid < nk) A.hits[q * nk + tid] = cnt[2 + tid];
  if (tid == 0) {
    A.best[q] = 1 + cnt[1];
    A.nans[q] = cnt[0];
    if (A.sqerr) A.sqerr[q] = sq[0];
  }
}

// every check that needs no pointer (siamese_eval.h, in its order)
int eval_shape_rc(int64_t m, int64_t n, int32_t nk) {
  if (m < 0 || n < 0 || nk < 1) return SG_ERR_ARG;
  if (nk > kEvalMaxK) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

int eval_size_rc(int64_t m, int64_t n) {
  if (n > kEvalMaxCols || m > kEvalMaxRows) return SG_ERR_UNSUPPORTED;
  return SG_OK;
}

}  // namespace

extern "C" {

int64_t sg_eval_rows_workspace_bytes(int64_t m, int64_t n, int32_t nk) {
  if (eval_shape_rc(m, n, nk) != SG_OK || nk > n - 1 || eval_size_rc(m, n) != SG_OK) return -1;
  return 0;
}

int32_t sg_eval_rows(const float *scores, int64_t m, int64_t n, int64_t ld,
                     const int32_t *true_rank, const double *true_sim, const int32_t *ks,
                     int32_t nk, int32_t *hits_out, int32_t *best_rank_out, double *sqerr_out,
                     int32_t *nan_out, void *workspace, sg_stream_t stream) {
  if (ld < 0) return SG_ERR_ARG;
  int rc = eval_shape_rc(m, n, nk);
  if (rc != SG_OK) return rc;
  if (!ks || ks[0] < 1 || ks[nk - 1] >= n) return SG_ERR_ARG;
  for (int c = 1; c < nk; ++c)
    if (ks[c] <= ks[c - 1]) return SG_ERR_ARG;
  rc = eval_size_rc(m, n);
  if (rc != SG_OK) return rc;
  if (ld < n || (true_sim == nullptr) != (sqerr_out == nullptr)) return SG_ERR_ARG;
  if (m == 0) return SG_OK;
  if (!scores || !true_rank || !hits_out || !best_rank_out || !nan_out) return SG_ERR_ARG;
  (void)workspace;
  EvalArgs A;
  A.scores = scores;
  A.tr = true_rank;
  A.tsim = true_sim;
  A.ld = ld;
  A.n = (int)n;
  A.nk = nk;
  for (int c = 0; c < kEvalMaxK; ++c) A.ks[c] = c < nk ? ks[c] : 0;
  A.hits = hits_out;
  A.best = best_rank_out;
  A.nans = nan_out;
  A.sqerr = sqerr_out;
  const size_t lds = (size_t)((n + 255) & ~(int64_t)255) * 4u;
  sg_allow_lds((const void *)sg_eval_rows_kernel, lds);
  hipLaunchKernelGGL(sg_eval_rows_kernel, dim3((unsigned)m), dim3(kEvalThreads), lds,
                     (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? SG_OK : SG_ERR_HIP;
}

}  // extern "C"
