/*
 * siamese_ged_knn.h — the k nearest database graphs of every query under exact graph edit
 * distance on libsiamese_hip.so, by filter and verify: the bipartite bounds of siamese_ged.h
 * for every pair of a query x database grid of a dense graph store, a per-row threshold from
 * them, and the budgeted branch and bound of siamese_ged_exact.h only on the pairs the bounds
 * cannot exclude, started from the threshold instead of the pair's own upper bound.
 *
 * Cost model, store, q_idx / db_idx, status_out and unservable entries are those of
 * siamese_ged.h; the search (state, children, h, traversal order, expansion count and the
 * per-pair max_expansions) is that of siamese_ged_exact.h.  Per query row i:
 *
 *   seed        (ub0, lb0) of every pair is what sg_ged_grid returns with both_orders = 1.  A
 *               database column the call cannot serve takes no part in any row.  n_valid is the
 *               number of servable columns and k' = min(k, n_valid).
 *   threshold   tau = the k'-th smallest ub0 of the row: k' graphs are known to lie within tau.
 *   filter      a pair is a candidate iff lb0 <= tau (every pair with ub0 <= tau is one).  A
 *               pair that is none has GED >= lb0 > tau and is in no top-k under any tie rule.
 *   verify      every candidate is searched as in siamese_ged_exact.h, except that the
 *               incumbent starts at c = min(ub0, tau + 1).  The search is skipped (0 expansions,
 *               seed bounds kept) where lb0 == ub0, where max(n1, n2) > 16 and when
 *               max_expansions == 0.  Otherwise
 *                 a complete map was found (cost < c): ub = its cost; lb = ub if the search
 *                     ended before the budget did, else lb0
 *                 none found, the search ended:  c == ub0: lb = ub = ub0 (proven)
 *                     c == tau + 1 < ub0: ub = ub0, lb = max(lb0, tau + 1): the pair is proven
 *                     to lie outside the threshold, its distance is not
 *                 none found, the budget ended it: ub = ub0, lb = lb0
 *               Where c == ub0 the pair's (ub, lb, expansions) are sg_ged_exact_grid's.
 *   select      the candidates in ascending (ub, column); the first k' are the row's output.
 *               With (d, s) the (ub, column) of the last one, certified = 1 iff every selected
 *               pair has lb == ub and every other candidate has lb > d, or lb == d and a column
 *               above s.  A certified row is the first k' entries of the row of exact
 *               distances in ascending (distance, column).  A row with k' == 0 and a servable
 *               query is certified (there is nothing to find).
 *
 * tau is fixed before any search starts and no threshold is shared between wavefronts, so all
 * outputs depend on the graphs, k and max_expansions alone, never on the launch shape, on the
 * position of a row or column in the grid or on its neighbours (beyond what the definition
 * above says), and two runs are bitwise equal.  The order of the compacted candidate list varies
 * from run to run; no output depends on it.
 *
 * Five stream-ordered steps and no host synchronisation: the entries, the seed (one wavefront
 * per pair), threshold and filter (one workgroup per row; ub0 <= 1056, so tau comes from a
 * counting pass in LDS), verify (one wavefront per candidate, lane mapping of
 * siamese_ged_exact.h; a fixed launch of 2048 wavefronts strides over the candidate count,
 * which stays on the device), select (one workgroup per row, k' rounds of a row-wide minimum).
 * Every loop is counted.
 *
 * The symbols' presence is how a caller detects the feature; sg_version() does not change
 * with them.
 */
#ifndef SIAMESE_GED_KNN_H
#define SIAMESE_GED_KNN_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 *   col_out        [m][k] int32: required.  Slot r: the column (index into db_idx) of the
 *                  r-th nearest candidate; slots k' .. k-1 read -1
 *   ub_out         [m][k] int32: required.  The cost of a real edit path of that pair; -1 in
 *                  slots k' .. k-1
 *   lb_out         [m][k] int32: required.  Equal to ub_out where the distance is proven; -1
 *                  in slots k' .. k-1
 *   certified_out  [m] int32: required.  1: the row is the true top-k' (see select)
 *   candidates_out [m] int32 or NULL: the pairs of the row that survived the filter
 *   expansions_out [m] int64 or NULL: the expansions spent on the row, summed over its pairs
 *   *status_out    as in siamese_ged.h.  A row whose query the call cannot serve reads -1 in
 *                  every slot, certified 0, candidates -1 and expansions -1.
 *
 * Checked in this order, before any HIP call:
 *   m or n negative                                           SG_ERR_ARG
 *   n_graphs < 0 or n_max < 1                                 SG_ERR_ARG
 *   n_max > 32                                                SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   k < 1                                                     SG_ERR_ARG
 *   k > 64                                                    SG_ERR_UNSUPPORTED
 *   max_expansions < 0                                        SG_ERR_ARG
 *   max_expansions > 2^24 (what bounds a launch)              SG_ERR_UNSUPPORTED
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store_adj, store_types, store_n, col_out, ub_out, lb_out,
 *   certified_out or workspace NULL                           SG_ERR_ARG
 *   workspace not 8-byte aligned                              SG_ERR_ARG
 *
 * workspace: sg_ged_knn_workspace_bytes(m, n, n_max, k) bytes, 8-byte aligned:
 *   16 + 4 * ((m + n) * W + 5 * m * n + 2 * m),  W = (2 * n_max + 4) & ~3
 * (the candidate count, the m + n entries of sg_ged_grid, per pair the seed's and the
 * verified (ub, lb) and a slot of the candidate list, per row tau and k'); 0 when m or n is 0
 * (`workspace` may be NULL then); -1 for m, n, n_max or k the call refuses.
 */
int64_t sg_ged_knn_workspace_bytes(int64_t m, int64_t n, int32_t n_max, int32_t k);
int32_t sg_ged_knn(const float *store_adj, const int32_t *store_types, const int32_t *store_n,
                   int32_t n_graphs, int32_t n_max, const int32_t *q_idx, int64_t m,
                   const int32_t *db_idx, int64_t n, int32_t k, int64_t max_expansions,
                   int32_t *col_out, int32_t *ub_out, int32_t *lb_out, int32_t *certified_out,
                   int32_t *candidates_out, int64_t *expansions_out, int32_t *status_out,
                   void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_GED_KNN_H */
