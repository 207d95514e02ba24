/*
 * siamese_embed_drop.h — embed-once training WITH dropout on libsiamese_hip.so: the node
 * stack of single graphs, forward and backward, under dropout masks keyed per graph.
 *
 * The reference draws its dropout masks per pair: every sess.run of a pair draws fresh
 * floor(keep_prob + U[0,1)) masks for both of its graphs (layers.py:334-336 for the sparse
 * first layer, tf.nn.dropout for the others; quirk A4).  A graph's embedding then depends on
 * its partner, the m x n block of pairs does not factor into m + n node stacks, and the
 * calls of siamese_embed_train.h refuse every model with effective dropout.
 *
 * GRAPH-KEYED MASKS — a deliberate deviation from quirk A4, of the same kind as the
 * inference mode of siamese_embed.h: the calls here draw ONE mask set per embedded entry
 * per call (seed), covering every node layer and the mask the NTN head applies to its input
 * vector (layers.py:282-310 through tf.nn.dropout).  Every pair of the block that an entry
 * takes part in sees that one mask set.  This is ordinary dropout in a batched Siamese
 * model; it is not what the reference's per-pair sess.run does.
 *
 * The contract.  A call embeds `count` entries; entry c has the global entry number
 * c' = entry_offset + c and is computed as SIDE c' & 1 OF UNIT c' >> 1:
 *     pk = sg_pair_key(sg_seed_key(seed), (uint32_t)(c' >> 1))
 * so every node-layer mask and the head-input mask of entry c is exactly the mask the
 * generic pair kernel (sg_forward / sg_fwd_bwd, path 0) draws for pair c' >> 1, side
 * c' & 1, under the same seed.  The embedding returned is the MASKED embedding
 *     where(keep(pk, head layer, side, e), e_c[e] / keep_prob, 0)
 * when the head is an NTN layer with dropout set; a Dot head or an NTN head without dropout
 * gets the plain embedding.  The masks depend on the seed, the entry number and the model;
 * they do not depend on which graph shares the wavefront, on the launch shape, or on how a
 * caller splits a call (entries 4 .. 8 with entry_offset = 4 are rows 4 .. 8 of the whole
 * call, bit for bit).  Because the head's mask is already in the embeddings, the grid calls
 * (sg_score_grid, sg_score_grid_fwd_bwd) run on them with a copy of the model whose
 * keep_prob is 1.
 *
 * model->keep_prob is honoured with the per-layer dropout flags; model->adj_dtype is still
 * ignored (the f32 graph store is read).  Models on the graph-store path (sg_model_validate
 * path 3) give SG_ERR_UNSUPPORTED, and so does a stack that does not fit the LDS, as in
 * sg_embed.  The calls of siamese_embed.h and siamese_embed_train.h keep their behaviour
 * and their refusals.
 *
 * Feature detection: sg_version() is unchanged by these entry points; a caller detects
 * them by the presence of the symbols below (dlsym / ctypes hasattr).
 *
 * Conventions are those of siamese_hip.h: caller-owned DEVICE buffers unless noted,
 * stream-ordered calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code.
 * Every entry point checks its arguments on the host before its first HIP call: a NULL
 * model, a negative count or entry_offset, an odd entry_offset (a call starts at side 0 of
 * a unit) and a keep_prob outside (0, 1] give SG_ERR_ARG.
 */
#ifndef SIAMESE_EMBED_DROP_H
#define SIAMESE_EMBED_DROP_H

#include "siamese_embed_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * sg_embed (siamese_embed.h) with graph-keyed dropout: emb_out [count][E] receives the
 * masked embeddings defined above.  store_*, n_graphs, n_max, graph_idx, params, status_out
 * are sg_embed's: a bad id sets SG_ERR_ARG and a bad node count SG_ERR_SHAPE in
 * *status_out, and that entry's row is written as zeros.  At keep_prob = 1 (or with no
 * layer's dropout set) the rows are sg_embed's, bit for bit.
 */
int32_t sg_embed_drop(const sg_model_t *model, const float *store_adj,
                      const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                      int32_t n_max, const int32_t *graph_idx, int64_t count,
                      int64_t entry_offset, const float *params, uint64_t seed, float *emb_out,
                      int32_t *status_out, sg_stream_t stream);

/*
 * sg_embed_bwd (siamese_embed_train.h) with graph-keyed dropout.  g_emb [count][E] is the
 * gradient with respect to the MASKED embedding sg_embed_drop returned for the same
 * entries, entry_offset and seed; the kernel applies the head mask and 1 / keep_prob to it,
 * reruns the masked forward of the stack and runs its backward under the same masks.
 * grad_out[0 .. head offset) receives the node layers' range exactly as sg_embed_bwd writes
 * it; the head's range is not touched.  An entry that cannot be embedded contributes
 * nothing.  count == 0 zeroes the range.  Not bitwise reproducible, as sg_embed_bwd.
 * workspace: sg_embed_drop_bwd_workspace_bytes(model, count) bytes, what
 * sg_embed_bwd_workspace_bytes gives for a model both calls serve; -1 for a model this call
 * does not serve or a negative count.
 */
int64_t sg_embed_drop_bwd_workspace_bytes(const sg_model_t *model, int64_t count);
int32_t sg_embed_drop_bwd(const sg_model_t *model, const float *store_adj,
                          const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                          int32_t n_max, const int32_t *graph_idx, int64_t count,
                          int64_t entry_offset, const float *params, uint64_t seed,
                          const float *g_emb, float *grad_out, int32_t *status_out,
                          void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_EMBED_DROP_H */
