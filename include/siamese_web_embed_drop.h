/*
 * siamese_web_embed_drop.h — embed-once training WITH dropout for graph-store (Web) models
 * on libsiamese_hip.so: the CSR node stack of single graphs, forward and backward, under
 * dropout masks keyed per graph (sg_model_validate path 3, BASELINE config C5).
 *
 * This is siamese_embed_drop.h restated for path 3.  The reference draws its dropout masks
 * per pair: every sess.run of a pair draws fresh floor(keep_prob + U[0,1)) masks for both of
 * its graphs (layers.py:334-336 for the sparse first layer, tf.nn.dropout for the others;
 * quirk A4).  A graph's embedding then depends on its partner, the m x n block of pairs
 * does not factor into m + n node stacks, and the calls of siamese_web_embed_train.h refuse
 * every model with effective dropout.
 *
 * GRAPH-KEYED MASKS — a deliberate deviation from quirk A4, of the same kind as the
 * inference mode of siamese_web_embed.h: the calls here draw ONE mask set per embedded entry
 * per call (seed), covering every node layer and the mask the NTN head applies to its input
 * vector (layers.py:282-310 through tf.nn.dropout).  Every pair of the block that an entry
 * takes part in sees that one mask set.  This is ordinary dropout in a batched Siamese
 * model; it is not what the reference's per-pair sess.run does.
 *
 * The contract.  A call embeds `count` entries; entry c has the global entry number
 * c' = entry_offset + c and is computed as SIDE c' & 1 OF UNIT c' >> 1:
 *     pk = sg_pair_key(sg_seed_key(seed), (uint32_t)(c' >> 1))
 * so every mask of entry c is bit for bit the mask sg_web_forward / sg_web_fwd_bwd draw for
 * pair c' >> 1, side c' & 1, at pair_offset = 0 under the same seed:
 *   - the sparse layer-0 mask on the node types,
 *   - the masks of layers 1 and 2,
 *   - the NTN-input mask (layer 4) on the node columns [0, N),
 *   - the layer-4 mask on the Padding columns [N, D) when padding_value != 0.
 * The embedding returned is the MASKED embedding, the vector x the pair kernel hands to its
 * NTN head:
 *     where(keep(pk, layer 4, side, e), e_c[e] / keep_prob, 0)
 * when the NTN layer has dropout set; the plain embedding otherwise.  The masks depend on
 * the seed, the entry number and the model; they do not depend on which entries share a
 * workgroup or size class, on the chunking inside the call, or on how a caller splits a
 * call (entries 4 .. 8 with entry_offset = 4 are rows 4 .. 8 of the whole call, bit for
 * bit).  Because the head's mask is already in the embeddings, the grid calls
 * (sg_web_score_grid, sg_web_score_grid_fwd_bwd, sg_web_search_topk) run on them with a
 * copy of the model whose keep_prob is 1.
 *
 * model->keep_prob is honoured with the per-layer dropout flags.  Models off path 3 give
 * SG_ERR_UNSUPPORTED, and so does a stack that does not fit the LDS, as in sg_web_embed.
 * The calls of siamese_web_embed.h and siamese_web_embed_train.h keep their behaviour and
 * their refusals.
 *
 * Feature detection: sg_version() is unchanged by these entry points; a caller detects
 * them by the presence of the symbols below (dlsym / ctypes hasattr).
 *
 * Conventions are those of siamese_hip.h: caller-owned DEVICE buffers unless noted,
 * stream-ordered calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code.
 * Every entry point checks its arguments on the host before its first HIP call: a NULL
 * model, a negative count or entry_offset, an odd entry_offset (a call starts at side 0 of
 * a unit) and a keep_prob outside (0, 1] give SG_ERR_ARG; then the checks of sg_web_embed /
 * sg_web_embed_bwd without the dropout refusal; count or entry_offset + count above 2^29
 * gives SG_ERR_UNSUPPORTED.
 */
#ifndef SIAMESE_WEB_EMBED_DROP_H
#define SIAMESE_WEB_EMBED_DROP_H

#include "siamese_web_embed_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * sg_web_embed (siamese_web_embed.h) with graph-keyed dropout: emb_out [count][ld],
 * ld = sg_web_embed_ld(model), receives the masked embeddings defined above in
 * sg_web_embed's layout (all ld columns written).  store, graph_idx, params, status_out are
 * sg_web_embed's: a bad id sets SG_ERR_ARG and a bad node count SG_ERR_SHAPE in
 * *status_out, and that entry's row is written as zeros.  At keep_prob = 1 (or with no
 * layer's dropout set) the rows are sg_web_embed's, bit for bit.  count == 0 is SG_OK with
 * no launch.
 * The instance kernel of the pair path keeps side s of unit u at row s·Cp + u of its
 * output, so the call stages the rows there and one kernel moves them to emb_out; that
 * takes more than sg_web_embed's workspace.
 * workspace: sg_web_embed_drop_workspace_bytes(model, count) bytes, -1 for a model off
 * path 3 or a count outside [0, 2^29].  With Dp = sg_web_embed_ld(model) and
 * ce = count rounded up to 2:
 *   4 · up64(ce · Dp)  +  sg_web_embed_workspace_bytes(model, count).
 */
int64_t sg_web_embed_drop_workspace_bytes(const sg_model_t *model, int64_t count);
int32_t sg_web_embed_drop(const sg_model_t *model, const sg_csr_store_t *store,
                          const int32_t *graph_idx, int64_t count, int64_t entry_offset,
                          const float *params, uint64_t seed, float *emb_out,
                          int32_t *status_out, void *workspace, sg_stream_t stream);

/*
 * sg_web_embed_bwd (siamese_web_embed_train.h) with graph-keyed dropout.  g_emb [count] rows
 * of stride ld_g (ld_g >= D) is the gradient with respect to the MASKED embedding
 * sg_web_embed_drop returned for the same entries, entry_offset and seed.  Per chunk of
 * cc = min(count, 1024) entries (1,024 is even: no unit straddles two chunks) the call
 * reruns the masked forward, which stores its keep bits and D2 rows, and runs the backward
 * instance kernel of the pair path under those bits; the kernel applies the head mask and
 * 1 / keep_prob to g_emb.  grad_out[0 .. offset of weights_W) receives the node layers'
 * range exactly as sg_web_embed_bwd writes it (one gradient row per workgroup, then one
 * fixed-order column sum); the head's range is not touched.  An entry that cannot be
 * embedded sets *status_out and contributes nothing.  count == 0 zeroes the range.  Two
 * calls on equal inputs on one device agree bitwise.  At keep_prob = 1 (or with no layer's
 * dropout set) the range is sg_web_embed_bwd's, bit for bit.
 * workspace: sg_web_embed_drop_bwd_workspace_bytes(model, count) bytes, -1 for a model off
 * path 3 or a count outside [0, 2^29].  With Dp, cc as above, ce = cc rounded up to 2 and
 * n_gcn the length of the node-layer range:
 *   4 · ( up64(512 · n_gcn)        gradient rows (a device with more than 512 CUs is refused)
 *       + 2 · up64(ce · Dp)        the chunk's embeddings and its rows of g_emb, side-major
 *       + up64(cc · Dp · 4)        keep bits, uint16 [2 cc][Dp][4]
 *       + up64(cc · Dp · 32)       D2 rows [2 cc][Dp][16]
 *       + up64(cc)                 the chunk's graph ids
 *       + sg_web_embed_workspace_bytes(model, cc) / 4 )   instance records and unit sort
 *   + 256.
 */
int64_t sg_web_embed_drop_bwd_workspace_bytes(const sg_model_t *model, int64_t count);
int32_t sg_web_embed_drop_bwd(const sg_model_t *model, const sg_csr_store_t *store,
                              const int32_t *graph_idx, int64_t count, int64_t entry_offset,
                              const float *params, uint64_t seed, const float *g_emb,
                              int64_t ld_g, float *grad_out, int32_t *status_out,
                              void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_WEB_EMBED_DROP_H */
