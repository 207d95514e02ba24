/*
 * siamese_ged.h — graph edit distance bounds on libsiamese_hip.so: the bipartite
 * approximation of Riesen & Bunke for every pair of a query x database grid of a dense graph
 * store, one wavefront per pair, with the certified lower bound of the same construction.
 *
 * Cost model (the graph-matching-toolkit's for the AIDS sets, doubled at alpha = 0.5 so every
 * distance is an integer): node insertion / deletion 1, node substitution 0 for equal type
 * and 1 otherwise, edge insertion / deletion 1, edge substitution 0.
 *
 * For graph 1 (n1 nodes) and graph 2 (n2 nodes), N = n1 + n2 <= 64, with t the store's type
 * entry, deg the number of off-diagonal non-zeros of the node's row of store_adj and an edge
 * between a != b iff adj[g][a][b] != 0:
 *
 *   C (N x N int32)   C[i][j]      = w [t1_i != t2_j] + |deg1_i - deg2_j|     i < n1, j < n2
 *                     C[i][n2 + i] = w + deg1_i                               deletion
 *                     C[n1 + j][j] = w + deg2_j                               insertion
 *                     2^20 elsewhere in the deletion and insertion blocks, 0 in the
 *                     (N - n1) x (N - n2) block of the two epsilon sides
 *   LSAP              shortest augmenting paths with row and column potentials, all int32:
 *                     rows enter in index order, the column argmin breaks ties to the smallest
 *                     column index, minv is updated on strict <, every loop is counted and
 *                     bounded by N
 *   ub(1->2)          w = 1; the cost of the edit path the assignment phi induces: deletions +
 *                     insertions + substituted nodes of different type + |E1| + |E2| -
 *                     2 #{(a, b) in E1 : phi(a), phi(b) != eps, (phi(a), phi(b)) in E2}
 *   ub                ub(1->2), or min(ub(1->2), ub(2->1)) with both_orders
 *   lb                w = 2 (every edge cost split over its two ends): ceil(opt / 2).  The
 *                     matrix of the swapped pair is the transpose, so it is solved once.
 *                     lb <= GED <= ub; where lb == ub the distance is exact.
 *
 * Results depend on the two graphs alone, never on the launch shape or on the pair's position
 * in the grid.
 *
 * Conventions are those of siamese_eval.h: caller-owned DEVICE buffers, stream-ordered calls,
 * no allocation, no host synchronisation, SG_OK or an SG_ERR_* code, arguments checked on the
 * host before the first HIP call.  The symbols' presence is how a caller detects the feature;
 * sg_version() does not change with them.
 */
#ifndef SIAMESE_GED_H
#define SIAMESE_GED_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The store is sg_embed's: store_adj [n_graphs][n_max][n_max] f32, store_types
 * [n_graphs][n_max], store_n [n_graphs].  q_idx [m] / db_idx [n] select store graphs (repeats
 * allowed); NULL means graphs 0 .. m-1 / 0 .. n-1.  Pair (i, j) is graph 1 = q_idx[i] against
 * graph 2 = db_idx[j].
 *
 *   ub_out  [m] rows of n int32, row stride ld: required
 *   lb_out  the same shape, or NULL (the lower bound is not computed then)
 *   map_out [m][n][n_max] int8 or NULL: phi of the 1->2 order (not of whichever order won the
 *           min): the graph-2 node of graph-1 node a, -1 for a deleted node and for every
 *           entry at and beyond n1
 *   *status_out (device int, may be NULL): an id outside the store sets SG_ERR_ARG, a node
 *           count outside [1, n_max] sets SG_ERR_SHAPE, as sg_embed does.  Every pair of such
 *           an entry reads ub = lb = -1 and map = -1; no other graph is substituted, and every
 *           other pair is unaffected.
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   n_graphs < 0 or n_max < 1                                 SG_ERR_ARG
 *   n_max > 32 (N <= 64: one lane per column)                 SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   both_orders neither 0 nor 1                               SG_ERR_ARG
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store_adj, store_types, store_n, ub_out or workspace NULL SG_ERR_ARG
 *
 * workspace: sg_ged_grid_workspace_bytes(m, n, n_max) bytes, 4-byte aligned (the adjacency
 * bit masks, types and node counts of the m + n entries, built once per call); 0 when m or n
 * is 0 (`workspace` may be NULL then); -1 for m, n, n_max the call refuses by the first,
 * third and fourth rule and for n_max < 1.
 */
int64_t sg_ged_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max);
int32_t sg_ged_grid(const float *store_adj, const int32_t *store_types, const int32_t *store_n,
                    int32_t n_graphs, int32_t n_max, const int32_t *q_idx, int64_t m,
                    const int32_t *db_idx, int64_t n, int32_t both_orders, int32_t *ub_out,
                    int64_t ld, int32_t *lb_out, int8_t *map_out, int32_t *status_out,
                    void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_GED_H */
