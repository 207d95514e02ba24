/*
 * siamese_ged_refine.h — local search on the node map on libsiamese_hip.so: the 2-exchange
 * refinement of the bipartite maps of siamese_ged.h (K-REFINE with K = 2) for every pair of a
 * query x database grid of a dense graph store, one wavefront per pair.  It lowers the upper
 * bound and proves nothing by itself: lb is the bipartite one.  Every servable pair
 * (n1, n2 <= 32) is refined.
 *
 * The name 'bpswap' the Python layer gives it is this project's; no toolkit value is claimed.
 *
 * Cost model, store, q_idx / db_idx, ld, status_out and every other convention are those of
 * siamese_ged.h.  Graph 1 (n1 nodes) is the query, graph 2 (n2 nodes) the database graph.  A
 * map phi sends each graph-1 node to a distinct graph-2 node or to -1 (deleted); its cost is
 *   deletions + insertions + type mismatches + |E1| + |E2|
 *     - 2 (edges of graph 1 whose image is an edge of graph 2).
 *
 *   seed        siamese_ged_exact.h's: ub12 with its map phi12, ub21 with phi21 turned into a
 *               1->2 map, and the bipartite lb.
 *   move (a, x) a in [0, n1), x in [0, n2), x != phi[a]: phi'[a] = x; if some b != a has
 *               phi[b] == x then phi'[b] = phi[a] (which may be -1); everything else stays.
 *               That is the exchange of two images, the move onto a free graph-2 node, the
 *               un-deletion of a node and the hand-over of an image to a deleted node.
 *               There is no move to -1 alone: deleting a mapped node a and inserting its image
 *               adds a deletion and an insertion (2), saves at most the type mismatch (1) and
 *               loses two for every kept edge at a, so it changes the cost by
 *               2 - mismatch + 2 (kept edges at a) >= 1 and never improves.
 *               (Both bipartite maps leave min(n1, n2) nodes mapped and no other move changes
 *               that number, so from these seeds an un-deletion finds no deleted node next to
 *               a free one; it is part of the rule all the same.)
 *   sweep       the exact cost of phi' for every legal move; the best move is the smallest
 *               (cost, a, x), compared in that order (two moves can give the same phi': the
 *               smaller a wins).  It is accepted iff its cost is strictly below the current
 *               cost; otherwise the start has reached a local optimum and ends.
 *   start       accepts at most max_moves moves.  Start 0 descends from phi12, start 1 from
 *               the inverse of phi21; both always run on a pair that is not skipped.
 *   result      the final state of start 0, or that of start 1 where its final cost is strictly
 *               lower: ub is that cost, map that map; lb = ub where ub equals the seed's lb,
 *               otherwise the seed's lb; moves = the accepted moves of both starts.
 *   skipped     a pair whose seed has lb == min(ub12, ub21), and every pair when
 *               max_moves == 0: moves = 0 and the result is the seed's by the same rule (phi12,
 *               or the inverse of phi21 where ub21 < ub12 strictly).
 *
 * Every loop is counted: an accepted move lowers the cost by at least 1 and the cost never
 * goes below lb, so a start makes at most min(max_moves, seed ub - lb) moves of at most
 * n1 * n2 <= 1024 evaluations.  Results, moves included, depend on the two graphs and max_moves
 * alone, never on the launch shape, on the pair's position in the grid or on its neighbours;
 * two runs are bitwise equal.
 *
 * The symbols' presence is how a caller detects the feature; sg_version() does not change
 * with them.
 */
#ifndef SIAMESE_GED_REFINE_H
#define SIAMESE_GED_REFINE_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 *   ub_out   [m] rows of n int32, row stride ld: required.  The cost of a real edit path,
 *            never above sg_ged_grid's ub with both_orders = 1.
 *   lb_out   the same shape: required.  sg_ged_grid's lb.
 *   map_out  [m][n][n_max] int8 or NULL: phi of graph 1 -> graph 2 of the path whose cost is
 *            ub_out: the graph-2 node of graph-1 node a, -1 for a deleted node and for every
 *            entry at and beyond n1
 *   moves_out [m] rows of n int32, row stride ld, or NULL: the moves accepted, both starts
 *   *status_out as in siamese_ged.h; every pair of an entry the call cannot serve reads
 *            ub = lb = -1, map = -1 and moves = -1, and every other pair is unaffected.
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   n_graphs < 0 or n_max < 1                                 SG_ERR_ARG
 *   n_max > 32                                                SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   max_moves < 0                                             SG_ERR_ARG
 *   max_moves > 4096                                          SG_ERR_UNSUPPORTED
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store_adj, store_types, store_n, ub_out, lb_out or
 *   workspace NULL                                            SG_ERR_ARG
 *
 * workspace: sg_ged_refine_grid_workspace_bytes(m, n, n_max) bytes, 4-byte aligned, by the
 * rules of sg_ged_grid_workspace_bytes (and the same size: the maps live in LDS).
 */
int64_t sg_ged_refine_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max);
int32_t sg_ged_refine_grid(const float *store_adj, const int32_t *store_types,
                           const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                           const int32_t *q_idx, int64_t m, const int32_t *db_idx, int64_t n,
                           int32_t max_moves, int32_t *ub_out, int64_t ld, int32_t *lb_out,
                           int8_t *map_out, int32_t *moves_out, int32_t *status_out,
                           void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_GED_REFINE_H */
