/*
 * siamese_ged_beam.h — beam-search graph edit distance on libsiamese_hip.so: a level-synchronous
 * beam over node maps for every pair of a query x database grid of a dense graph store, one
 * wavefront per pair, seeded with the bipartite bounds of siamese_ged.h.  A pair runs at most n1
 * levels of at most `width` states, so its run time has a ceiling, and every servable pair
 * (n1, n2 <= 32) is searched.  Where no state was ever dropped because of the width the beam was
 * a complete search and the distance is proven (lb == ub), in the sense of siamese_ged_exact.h;
 * elsewhere the best upper bound found and the bipartite lower bound are returned.
 *
 * This is not the graph-matching-toolkit's beam search (best-first over a truncated OPEN list):
 * its values are not claimed to be that program's.
 *
 * Cost model, store, q_idx / db_idx, ld, status_out and every other convention are those of
 * siamese_ged.h.  Graph 1 (n1 nodes) is the query, graph 2 (n2 nodes) the database graph.
 *
 *   seed        siamese_ged_exact.h's: ub of both assignment orders, the bipartite lb, and the
 *               map phi12, or the inverse of phi21 where ub21 < ub12 strictly.  The incumbent is
 *               the seed's ub; it does not change during the levels (complete maps appear only
 *               at the last level).
 *   skipped     the search does not run, expanded = 0 and (ub, lb, map) is the seed, for a pair
 *               with seed lb == ub and for every pair when width == 0.  There is no 16-node
 *               limit.
 *   state, child, step cost, h
 *               exactly siamese_ged_exact.h's: graph-1 nodes are mapped in index order, each to
 *               an unused graph-2 node or to epsilon; h is the type-multiset term plus
 *               |e1r - e2r|; f = g + h of a complete map is its exact cost.
 *   level k     k = 0 .. n1 - 1.  Level 0 holds the root alone; slot p is a state's rank within
 *               its level.  Every state of the level is expanded (one expansion each).  A child
 *               with f >= incumbent is discarded (pruning, not truncation).  The surviving
 *               children of the whole level are ordered by f ascending, then parent slot p
 *               ascending, then graph-2 index ascending with epsilon last; every key is unique.
 *               For k < n1 - 1 the first `width` of them become level k + 1, in that order; more
 *               than `width` survivors mark the pair truncated.  At k = n1 - 1 the survivors are
 *               complete maps: the first one, if any, is the result (ub = f, map = its map).
 *               An empty level ends the search.
 *   result      ub = min(seed ub, best leaf); map = the map of the path that costs ub, always;
 *               lb = ub if the search ran and the pair was never truncated (the pruning is
 *               admissible, so the search was complete), otherwise the seed's lb;
 *               expanded = the states expanded, at most 1 + (n1 - 1) * width.
 *
 * Every loop is counted: at most 32 levels of at most 128 states of at most 33 children.
 * Results, expanded included, depend on the two graphs and the width alone, never on the launch
 * shape, on the pair's position in the grid or on its neighbours; two runs are bitwise equal.
 *
 * The symbols' presence is how a caller detects the feature; sg_version() does not change
 * with them.
 */
#ifndef SIAMESE_GED_BEAM_H
#define SIAMESE_GED_BEAM_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 *   ub_out   [m] rows of n int32, row stride ld: required.  The cost of a real edit path,
 *            never above sg_ged_grid's ub with both_orders = 1.
 *   lb_out   the same shape: required.  Equal to ub_out where the distance is proven (the
 *            bipartite bounds met, or the beam was never truncated), otherwise sg_ged_grid's lb.
 *   map_out  [m][n][n_max] int8 or NULL: phi of graph 1 -> graph 2 of the path whose cost is
 *            ub_out: the graph-2 node of graph-1 node a, -1 for a deleted node and for every
 *            entry at and beyond n1
 *   expanded_out [m] rows of n int32, row stride ld, or NULL: the states expanded
 *   *status_out as in siamese_ged.h; every pair of an entry the call cannot serve reads
 *            ub = lb = -1, map = -1 and expanded = -1, and every other pair is unaffected.
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   n_graphs < 0 or n_max < 1                                 SG_ERR_ARG
 *   n_max > 32                                                SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   width < 0                                                 SG_ERR_ARG
 *   width > 128 (what the wavefront's LDS holds)              SG_ERR_UNSUPPORTED
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store_adj, store_types, store_n, ub_out, lb_out or
 *   workspace NULL                                            SG_ERR_ARG
 *
 * workspace: sg_ged_beam_grid_workspace_bytes(m, n, n_max) bytes, 4-byte aligned, by the rules
 * of sg_ged_grid_workspace_bytes (and the same size: the beam lives in LDS).
 */
int64_t sg_ged_beam_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max);
int32_t sg_ged_beam_grid(const float *store_adj, const int32_t *store_types,
                         const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                         const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                         int32_t width, int32_t *ub_out, int64_t ld, int32_t *lb_out,
                         int8_t *map_out, int32_t *expanded_out, int32_t *status_out,
                         void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_GED_BEAM_H */
