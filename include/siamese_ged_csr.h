/*
 * siamese_ged_csr.h — graph edit distance bounds on libsiamese_hip.so for graph-store (CSR)
 * graphs of up to 512 nodes: the bipartite approximation of Riesen & Bunke for every pair of a
 * query x database grid of a sg_csr_store_t, one wavefront per pair, with the certified lower
 * bound of the same construction.
 *
 * Cost model (the graph-matching-toolkit's for the AIDS sets, doubled at alpha = 0.5 so every
 * distance is an integer): node insertion / deletion 1, node substitution 0 for equal type
 * and 1 otherwise, edge insertion / deletion 1, edge substitution 0.
 *
 * The graphs: graph g of the store has n = node_off[g + 1] - node_off[g] nodes; node a of it
 * has type types[node_off[g] + a] and the CSR row row_ptr[node_off[g] + a] ..
 * row_ptr[node_off[g] + a + 1] of (col, val) entries, col local to the graph.  An edge joins
 * a != b iff the store holds an entry (a, b) with val != 0; deg counts those entries of the
 * node's row (diagonal entries and stored zeros are no edges).  The store must be symmetric
 * (an entry (a, b) with val != 0 has an entry (b, a) with val != 0), every row's columns must
 * be strictly ascending and inside [0, n) (the induced cost searches a row by bisection), and
 * every type must lie in [0, 2^22).
 *
 * For graph 1 (n1 nodes) and graph 2 (n2 nodes), N = n1 + n2 <= 1024, with t the type and deg
 * the degree of a node:
 *
 *   C (N x N int32)   C[i][j]      = w [t1_i != t2_j] + |deg1_i - deg2_j|     i < n1, j < n2
 *                     C[i][n2 + i] = w + deg1_i                               deletion
 *                     C[n1 + j][j] = w + deg2_j                               insertion
 *                     F = 2^21 (forbidden) elsewhere in the deletion and insertion blocks,
 *                     0 in the (N - n1) x (N - n2) block of the two epsilon sides
 *   LSAP              shortest augmenting paths with row and column potentials, all int32:
 *                     rows enter in index order; a round takes the unmarked column of smallest
 *                     minv, ties to the smallest column index; minv is replaced on strict <;
 *                     every loop is counted and bounded by N
 *   ub(1->2)          w = 1; the cost of the edit path the assignment phi induces: deletions +
 *                     insertions + substituted nodes of different type + |E1| + |E2| -
 *                     2 #{(a, b) in E1 : phi(a), phi(b) != eps, (phi(a), phi(b)) in E2}
 *   ub                ub(1->2), or min(ub(1->2), ub(2->1)) with both_orders
 *   lb                w = 2 (every edge cost split over its two ends): ceil(opt / 2).  The
 *                     matrix of the swapped pair is the transpose, so it is solved once.
 *                     lb <= GED <= ub; where lb == ub the distance is exact.
 *
 * Integer widths.  Let K = 2 + 511 = 513 bound every finite entry (w <= 2, deg <= 511) and
 * D = 1024 K = 525312.  Every row has a finite entry in a column of its own (its deletion
 * column, or the insertion column of an epsilon row), so the first k rows have an assignment
 * of cost <= k K <= D, and with opt_k the optimum of the first k rows, 0 <= opt_k <= D.
 *   - The distance at which row i's search ends is opt_(i+1) - opt_i, in [0, D]: every column
 *     that a round takes has minv <= D.
 *   - Column potentials only fall, by at most that distance per row: -D <= v <= 0.  A row
 *     assigned through a finite entry has u = C - v, so 0 <= u <= K + D.
 *   - A forbidden entry's minv is at least F - (K + D) = 1571327 > D, so no round takes one and
 *     no assignment holds one (F > 2 D + K is what this needs).
 *   - Every minv is at most F + D = 2622464 < 2^22, and never negative.  The argmin is the
 *     wave-wide minimum of the uint32 key minv << 10 | column, at most 2622464 * 1024 + 1023 <
 *     2^32 - 1 (the key of a marked column): its order is (minv, column) lexicographic.
 *   - opt <= D; every sum above fits int32 with room to spare.
 *
 * Results depend on the two graphs alone, never on the launch shape or on the pair's position
 * in the grid.
 *
 * Conventions are those of siamese_eval.h: caller-owned DEVICE buffers, stream-ordered calls,
 * no allocation, no host synchronisation, SG_OK or an SG_ERR_* code, arguments checked on the
 * host before the first HIP call.  The symbols' presence is how a caller detects the feature;
 * sg_version() does not change with them.
 */
#ifndef SIAMESE_GED_CSR_H
#define SIAMESE_GED_CSR_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * store is the HOST struct of siamese_hip.h holding DEVICE pointers (max_nnz is not read).
 * q_idx [m] / db_idx [n] select store graphs (repeats allowed); NULL means graphs 0 .. m-1 /
 * 0 .. n-1.  Pair (i, j) is graph 1 = q_idx[i] against graph 2 = db_idx[j].
 *
 *   ub_out  [m] rows of n int32, row stride ld: required
 *   lb_out  the same shape, or NULL (the lower bound is not computed then)
 *   map_out [m][n][n_max] int16 or NULL (n_max the struct's): phi of the 1->2 order (not of
 *           whichever order won the min): the graph-2 node of graph-1 node a, -1 for a deleted
 *           node and for every entry at and beyond n1
 *   *status_out (device int, may be NULL): an id outside the store sets SG_ERR_ARG, a node
 *           count outside [1, n_max] or a type outside [0, 2^22) sets SG_ERR_SHAPE.  Every pair
 *           of such an entry reads ub = lb = -1 and map = -1; no other graph is substituted,
 *           and every other pair is unaffected.
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   store->n_graphs < 0 or store->n_max < 1                   SG_ERR_ARG
 *   store->n_max > 512 (N <= 1024: 16 columns per lane)       SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   both_orders neither 0 nor 1                               SG_ERR_ARG
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store, its node_off, types, row_ptr, col or val, ub_out or workspace NULL   SG_ERR_ARG
 * (a NULL store has no n_graphs and n_max to check: the second and third rule pass it on)
 *
 * workspace: sg_csr_ged_grid_workspace_bytes(m, n, n_max) bytes, 4-byte aligned (per q / db
 * entry one packed (type, degree) word per node, the node count or -1 and the graph id, built
 * once per call); 0 when m or n is 0 (`workspace` may be NULL then); -1 for m, n, n_max the
 * call refuses by the first, third and fourth rule and for n_max < 1.
 */
int64_t sg_csr_ged_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max);
int32_t sg_csr_ged_grid(const sg_csr_store_t *store, const int32_t *q_idx, int64_t m,
                        const int32_t *db_idx, int64_t n, int32_t both_orders,
                        int32_t *ub_out, int64_t ld, int32_t *lb_out, int16_t *map_out,
                        int32_t *status_out, void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_GED_CSR_H */
