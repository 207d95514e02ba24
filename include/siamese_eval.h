/*
 * siamese_eval.h — device-side evaluation of the test matrix on libsiamese_hip.so: the
 * per-query integer counts behind ap@k and MRR and the squared-error sum behind "mse", from
 * the float32 score matrix sg_score_grid / sg_web_score_grid leave in device memory, in one
 * launch and without a sort.
 *
 * For query row q with scores s[j], true tie-best ranks tr[j] = #{j' : d[j'] < d[j]} (the
 * caller computes them once from the true distances) and the k's ks[0 .. nk):
 *
 *   p[j]       = #{j' : s[j'] > s[j] or (s[j'] == s[j] and j' > j)}
 *                the position of j in a stable ascending sort of the row, reversed (score
 *                descending, ties to the LARGER column; -0 == +0)
 *   hits[q][c] = #{j : tr[j] < ks[c] and p[j] < ks[c]}
 *                |tie-inclusive true top-k ∩ predicted top-k|; ap@k = mean_q hits / k
 *   best[q]    = 1 + #{j' : s[j'] > max{s[t] : tr[t] == 0}}
 *                the best tie-resolved predicted rank among the true top-1 graphs;
 *                MRR = 1 / hmean(best)
 *   sqerr[q]   = Σ_j (true_sim[q][j] − (double)s[j])², in float64, summed in a fixed order
 *                (the same bits from run to run); "mse" = sqrt(Σ_q sqerr[q]) / (m · n)
 *   nan[q]     = #{j : s[j] is NaN}.  A NaN score is outside the contract: when nan[q] != 0
 *                the other outputs of row q are unspecified.
 *
 * Conventions are those of siamese_search.h: caller-owned DEVICE buffers, stream-ordered
 * calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code, arguments
 * checked on the host before the first HIP call.  The symbols' presence is how a caller
 * detects the feature; sg_version() does not change with them.
 */
#ifndef SIAMESE_EVAL_H
#define SIAMESE_EVAL_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * scores [m] rows of n floats, row stride ld; true_rank [m][n]; true_sim [m][n] or NULL (no
 * sqerr); ks a HOST array of nk k's; hits_out [m][nk]; best_rank_out [m], 1-based;
 * sqerr_out [m], NULL iff true_sim is NULL (it is not written then); nan_out [m].
 * One workgroup per row keeps the row in LDS, so n <= 32768 (128 KB).
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   nk < 1                                                    SG_ERR_ARG
 *   nk > 16                                                   SG_ERR_UNSUPPORTED
 *   ks NULL, ks[0] < 1, ks not strictly ascending,
 *   or ks[nk-1] >= n                                          SG_ERR_ARG
 *   n > 32768                                                 SG_ERR_UNSUPPORTED
 *   m > 2^29                                                  SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   exactly one of true_sim and sqerr_out NULL                SG_ERR_ARG
 *   m == 0                                                    SG_OK, no work
 *   scores, true_rank, hits_out, best_rank_out or nan_out NULL    SG_ERR_ARG
 *
 * workspace: sg_eval_rows_workspace_bytes(m, n, nk) bytes: 0 (the kernel needs none and
 * `workspace` may be NULL; the query is kept so the call reads like the others), or -1 for
 * arguments the call refuses whatever ks holds: the rules above on m, n and nk, and
 * nk > n - 1 (no strictly ascending ks within [1, n) exists).
 */
int64_t sg_eval_rows_workspace_bytes(int64_t m, int64_t n, int32_t nk);
int32_t sg_eval_rows(const float *scores, int64_t m, int64_t n, int64_t ld,
                     const int32_t *true_rank, const double *true_sim, const int32_t *ks,
                     int32_t nk, int32_t *hits_out, int32_t *best_rank_out, double *sqerr_out,
                     int32_t *nan_out, void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_EVAL_H */
