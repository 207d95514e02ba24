/*
 * siamese_mcs.h — maximum common induced subgraph under a budget on libsiamese_hip.so: a
 * depth-first McSplit search (McCreesh, Prosser, Trimble 2017) for every pair of a query x
 * database grid of a dense graph store, one wavefront per pair.  The search counts its
 * expansions and stops at max_expansions, so a pair's run time has a ceiling: where the search
 * finishes the size is proven (size == bound), elsewhere the largest common subgraph found so
 * far and the root's upper bound are returned.
 *
 * Store, q_idx / db_idx, ld, status_out and every other convention are those of siamese_ged.h.
 * Graph 1 (n1 nodes, types t1, N1[a] the neighbour set of node a, edges E1) is the query,
 * graph 2 the database graph.
 *
 *   common      an injective partial map phi of graph-1 nodes to graph-2 nodes with
 *   induced     t1[a] == t2[phi(a)] for every mapped a and, for mapped a != c, (a, c) in E1 iff
 *   subgraph    (phi(a), phi(c)) in E2.  Its size is the number of mapped nodes, its edges are
 *               the edges of E1 with both ends mapped.  There are no edge labels.  With
 *               connected = 1 the mapped graph-1 nodes must also induce a connected subgraph.
 *   class       (L, R, adj): a non-empty set of graph-1 nodes, a non-empty set of graph-2
 *               nodes and one bit, set when the class's nodes are adjacent to a mapped node.
 *   state       the map so far, M, and an ordered list of classes.  The L of a state's classes
 *               are disjoint, so a state has at most n1 <= 32 classes.
 *   root        M empty; one class per type that occurs in both graphs, in the order of the
 *               smallest graph-1 node of the type, adj = 0.  ub0 = the sum of min(|L|, |R|)
 *               over the root's classes.  With no common type ub0 = 0: the pair is proven at
 *               size 0 with 0 expansions, whatever the budget.
 *   bound       of a state: |M| + the sum of min(|L|, |R|) over its classes.
 *   expansion   the generation of one state's children; the count starts at 0.  Before each
 *               expansion: if the count equals max_expansions the search stops, unproven.  An
 *               expansion that finds no class to select counts like any other.
 *   selection   the class of smallest max(|L|, |R|), ties to the earliest in the list; with
 *               connected = 1 and |M| > 0 among the classes with adj = 1 only, and a state
 *               that has none has no children.  v is the lowest node of the class's L.
 *   children    v -> w for every w of the class's R, ascending; last "v unmatched": v leaves
 *               the class's L, the class is dropped where L empties (the others keep their
 *               order and their adj), M stays.
 *   child       the classes of v -> w: for every old class in list order, with v taken out of
 *   classes     L and w out of R first, (L & N1[v], R & N2[w], adj = 1), then (L \ N1[v],
 *               R \ N2[w], the old adj); only the parts with both sets non-empty are kept.
 *   traversal   depth first from the root.  Before each child is generated: if the incumbent
 *               equals ub0 the search ends, proven.  A child v -> w whose |M| exceeds the
 *               incumbent becomes the incumbent and its map is recorded; then a child (of
 *               either kind) is expanded at once iff its bound exceeds the incumbent at that
 *               moment.  After a state's last child the search returns to its parent.
 *   proof       the pair is proven iff ub0 was reached, or the root's children ran out before
 *               the budget did.
 *
 * Every loop is counted: the stack has at most 32 levels (every level decides one graph-1
 * node, and an expanded state has a class left), a level at most 33 children, the search at
 * most max_expansions <= 2^24 expansions.  Results, expansions included, depend on the two
 * graphs, connected and the budget alone, never on the launch shape, on the pair's position in
 * the grid or on its neighbours; two runs are bitwise equal.
 *
 * This is the textbook problem, specified exactly.  It is not the connected maximum common
 * edge subgraph over atom and bond labels of the chorus library (MCS-DR) the reference calls,
 * and that program's values are not claimed.
 *
 * The symbols' presence is how a caller detects the feature; sg_version() does not change
 * with them.
 */
#ifndef SIAMESE_MCS_H
#define SIAMESE_MCS_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 *   size_out  [m] rows of n int32, row stride ld: required.  The incumbent: always the size of
 *             a real common induced subgraph (connected with connected = 1), 0 at the start.
 *   bound_out the same shape: required.  Equal to size_out where the size is proven, otherwise
 *             ub0: size == bound is the proof flag.
 *   edges_out the same shape, or NULL: the edges of the incumbent's map
 *   map_out   [m][n][n_max] int8 or NULL: the incumbent's phi: the graph-2 node of graph-1
 *             node a, -1 for an unmapped node and for every entry at and beyond n1
 *   expansions_out [m] rows of n int64, row stride ld, or NULL: the expansions spent
 *   *status_out as in siamese_ged.h; every pair of an entry the call cannot serve reads
 *             size = bound = edges = -1, map = -1 and expansions = -1, and every other pair is
 *             unaffected.
 *
 * Checked in this order, before any HIP call:
 *   m, n or ld negative                                       SG_ERR_ARG
 *   n_graphs < 0 or n_max < 1                                 SG_ERR_ARG
 *   n_max > 32                                                SG_ERR_UNSUPPORTED
 *   m > 2^24, n > 2^24 or m * n > 2^32                        SG_ERR_UNSUPPORTED
 *   ld < n                                                    SG_ERR_ARG
 *   connected neither 0 nor 1                                 SG_ERR_ARG
 *   max_expansions < 0                                        SG_ERR_ARG
 *   max_expansions > 2^24 (what bounds a launch)              SG_ERR_UNSUPPORTED
 *   m == 0 or n == 0                                          SG_OK, no work
 *   store_adj, store_types, store_n, size_out, bound_out or
 *   workspace NULL                                            SG_ERR_ARG
 *
 * workspace: sg_mcs_grid_workspace_bytes(m, n, n_max) bytes, 4-byte aligned, by the rules of
 * sg_ged_grid_workspace_bytes (and the same size).
 */
int64_t sg_mcs_grid_workspace_bytes(int64_t m, int64_t n, int32_t n_max);
int32_t sg_mcs_grid(const float *store_adj, const int32_t *store_types, const int32_t *store_n,
                    int32_t n_graphs, int32_t n_max, const int32_t *q_idx, int64_t m,
                    const int32_t *db_idx, int64_t n, int32_t connected, int64_t max_expansions,
                    int32_t *size_out, int64_t ld, int32_t *bound_out, int32_t *edges_out,
                    int8_t *map_out, int64_t *expansions_out, int32_t *status_out,
                    void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_MCS_H */
