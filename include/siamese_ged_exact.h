/*
 * siamese_ged_exact.h — exact graph edit distance under a budget on libsiamese_hip.so: a
 * depth-first branch and bound over node maps for every pair of a query x database grid of a
 * dense graph store, one wavefront per pair, seeded with the bipartite bounds of siamese_ged.h.
 * The search counts its expansions and stops at max_expansions, so a pair's run time has a
 * ceiling: where the search finishes the distance is proven (lb == ub), elsewhere the best
 * upper bound found so far and the bipartite lower bound are returned.
 *
 * Cost model, store, q_idx / db_idx, ld, status_out and every other convention are those of
 * siamese_ged.h.  Graph 1 (n1 nodes, types t1, edges E1) is the query, graph 2 the database
 * graph.
 *
 *   seed        ub12, phi12 = ub(1->2) and its assignment, ub21, phi21 = ub(2->1) and its
 *               assignment, lb: siamese_ged.h's.  The incumbent is min(ub12, ub21); its map
 *               is phi12, or, where ub21 < ub12 strictly, the inverse of phi21 (node a maps
 *               to the b with phi21[b] == a, else to epsilon).
 *   skipped     the search does not run, expansions = 0 and (ub, lb, map) is the seed, for a
 *               pair with lb == ub already, for a pair with max(n1, n2) > 16, and for every
 *               pair when max_expansions == 0.
 *   state       depth k: graph-1 nodes 0 .. k-1 are mapped, in index order, each to a graph-2
 *               node no other uses or to epsilon (deleted).  g is the cost so far.
 *   child       of a state at depth k: node k to an unused graph-2 node j, or to epsilon.
 *               Its step cost: to j, [t1_k != t2_j] plus, for every a < k, 1 if exactly one
 *               of (k, a) in E1 and (j, phi(a)) in E2 holds (phi(a) = epsilon: the second
 *               never holds); to epsilon, 1 plus the number of a < k with (k, a) in E1.
 *   h           of a state (depth k, used graph-2 nodes U), admissible:
 *               max(r1, r2) - |multiset intersection of the types of nodes k .. n1-1 and of
 *               the graph-2 nodes outside U|, r1 = n1 - k, r2 = n2 - |U|, plus |e1r - e2r|,
 *               e1r = the edges of E1 with an end >= k, e2r = the edges of E2 with an end
 *               outside U.  At depth n1 h is the cost of inserting the graph-2 nodes outside
 *               U and their edges, so f = g + h of a complete map is its exact cost.
 *   expansion   the generation of one state's children; the count starts at 0.  Before each
 *               expansion: if the count equals max_expansions the search stops, unproven.
 *   traversal   the root (depth 0, g = 0) is expanded; the children of an expanded state are
 *               taken in ascending f = g + h, ties to the smaller graph-2 index, epsilon
 *               last; the first child with f >= incumbent (the incumbent at that moment) ends
 *               the state and the search returns to its parent.  A child taken at depth
 *               n1 - 1 is a complete map: it becomes the incumbent (cost f) and is not
 *               expanded; every other child taken is expanded at once (depth first).
 *   proof       the pair is proven iff the root's children ended before the budget did; then
 *               lb = ub = the incumbent.  Otherwise ub = the incumbent and lb = the seed's.
 *
 * Every loop is counted: the stack has at most 16 levels, a level at most 17 children, the
 * search at most max_expansions <= 2^24 expansions.  Results, expansions included, depend on
 * the two graphs and the budget alone, never on the launch shape, on the pair's position in
 * the grid or on its neighbours; two runs are bitwise equal.
 *
 * The symbols' presence is how a caller detects the feature; sg_version() does not change
 * with them.
 */
#ifndef SIAMESE_GED_EXACT_H
#define SIAMESE_GED_EXACT_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 *   ub_out   [m] rows of n int32, row stride ld: required.  The cost of a real edit path,
 *            never above sg_ged_grid's ub with both_orders = 1.
 *   lb_out   the same shape: required.  Equal to ub_out where the search proved the distance
 *            (or the bipartite bounds met), otherwise sg_ged_grid's lb: lb == ub is the
 *            "exact" flag.
 *   map_out  [m][n][n_max] int8 or NULL: phi of graph 1 -> graph 2 of the path whose cost is
 *            ub_out (the induced cost of map_out equals ub_out, always): the graph-2 node of
 *            graph-1 node a, -1 for a deleted node and for every entry at and beyond n1
 *   expansions_out [m] rows of n int64, row stride ld, or NULL: the expansions spent
 *   *status_out as in siamese_ged.h; every pair of an entry the call cannot serve reads
 *            ub = lb = -1, map = -1 and expansions = -1, and every other pair is unaffected.
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   n_graphs < 0 or n_max < 1                                 SG_ERR_ARG
 *   n_max > 32                                                SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   max_expansions < 0                                        SG_ERR_ARG
 *   max_expansions > 2^24 (what bounds a launch)              SG_ERR_UNSUPPORTED
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store_adj, store_types, store_n, ub_out, lb_out or
 *   workspace NULL                                            SG_ERR_ARG
 *
 * workspace: sg_ged_exact_grid_workspace_bytes(m, n, n_max) bytes, 4-byte aligned, by the
 * rules of sg_ged_grid_workspace_bytes (and the same size).
 */
int64_t sg_ged_exact_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max);
int32_t sg_ged_exact_grid(const float *store_adj, const int32_t *store_types,
                          const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                          const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                          int64_t max_expansions, int32_t *ub_out, int64_t ld, int32_t *lb_out,
                          int8_t *map_out, int64_t *expansions_out, int32_t *status_out,
                          void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_GED_EXACT_H */
