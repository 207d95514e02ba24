/*
 * siamese_embed_train.h — embed-once training on libsiamese_hip.so: the adjoint of the
 * m x n NTN score grid and the backward of the node stack of single graphs.
 *
 * With dropout off a graph's node stack does not depend on its partner, and the NTN head
 * (layers.py:282-310) factors per query, m_k(i, j) = [e_j, 1] · Q_i[:, k] (siamese_embed.h).
 * The loss of an m x n block of pairs therefore needs m + n node-stack forwards, one grid
 * forward + backward (the loss gradient flows back through the grid to the m + n
 * embeddings), and one node-stack backward per graph, instead of m·n pair forwards and
 * backwards:
 *     sg_embed (siamese_embed.h)  →  sg_score_grid_fwd_bwd  →  [sum the query-role and
 *     database-role embedding gradients of each graph]  →  sg_embed_bwd
 * leaves the same Σ ∂loss/∂θ in grad_out as sg_fwd_bwd over the m·n pairs (head range from
 * the grid call, node-layer range from sg_embed_bwd), up to fp32 summation order.
 *
 * DROPOUT 0 ONLY.  The reference draws its dropout masks per pair (quirk A4), so with
 * dropout on a graph's node stack does depend on its partner and the factorisation does not
 * hold.  Unlike the inference calls of siamese_embed.h, which read model->keep_prob as 1,
 * both calls here REFUSE (SG_ERR_UNSUPPORTED) a model in which any layer, the head
 * included, has an effective keep probability below 1 (layer.dropout != 0 and a
 * model->keep_prob whose plan threshold is not 65536): nobody should optimise an objective
 * other than the one they asked for.  model->adj_dtype is ignored (the f32 graph store is
 * read).  Models on the graph-store path (sg_model_validate path 3) give
 * SG_ERR_UNSUPPORTED as well.
 *
 * Feature detection: sg_version() is unchanged by these entry points; a caller detects
 * them by the presence of the symbols below (dlsym / ctypes hasattr).
 *
 * Conventions are those of siamese_hip.h: caller-owned DEVICE buffers unless noted,
 * stream-ordered calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code.
 * Every entry point checks its arguments on the host before its first HIP call.
 */
#ifndef SIAMESE_EMBED_TRAIN_H
#define SIAMESE_EMBED_TRAIN_H

#include "siamese_embed.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Forward, loss and backward of the NTN head over the grid of (query i as graph 1,
 * database j as graph 2), emb_q [m][D], emb_db [n][D], D = the NTN input_dim.
 *   labels [m][ld_labels] (ld_labels >= n): y of pair (i, j); read by the aligned loss only
 *     (may be NULL for the broadcast loss).
 *   batch_total, y_stats (device {ȳ, ½Σ(y−ȳ)²}), add_label_term: as in sg_fwd_bwd.  The
 *     broadcast loss (model_mse.py:145-151) is ½Σ(ŷ−ȳ)² (+ y_stats[1] when add_label_term),
 *     the aligned loss ½Σ(ŷ−y)²/batch_total; the sums run over the m·n pairs of this call.
 *   s_out [m][ld_s] (ld_s >= n; may be NULL): pre-activation scores, columns j >= n of a
 *     row are not written.
 *   g_emb_q [m][D], g_emb_db [n][D]: ∂loss/∂embedding.
 *   grad_out [n_params]: only the head's variables are written (weights_W, weights_V,
 *     weights_U, bias: the last variables of the flat vector); the node-layer range in
 *     front of them is not touched (sg_embed_bwd writes it).
 *   loss_out [1] (may be NULL).
 * Serves what sg_score_grid serves: the NTN head with D <= 31 and feature_map_dim <= 16,
 * both ntn_modes, every inneract and final activation, bias on or off; SG_ERR_UNSUPPORTED
 * for the Dot head, larger heads, path 3 and any effective dropout.  m == 0 or n == 0 is
 * SG_OK and writes nothing.
 * Deterministic: per-workgroup partials are summed in a fixed order and no float atomics
 * are used, so two calls on equal inputs give bitwise equal outputs.
 * workspace: sg_score_grid_bwd_workspace_bytes(model, m, n) bytes; -1 for a model the call
 * does not serve and for m or n above the launch limit (2^29).  The larger part is one
 * partial of every query table's gradient per block of 64 database rows:
 * ceil(n / 64) · m · Dp · 64 bytes, Dp = D + 1 rounded up to 4.
 */
int64_t sg_score_grid_bwd_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n);
int32_t sg_score_grid_fwd_bwd(const sg_model_t *model, const float *emb_q, const float *emb_db,
                              int64_t m, int64_t n, const float *params, const float *labels,
                              int64_t ld_labels, int64_t batch_total, const float *y_stats,
                              int32_t add_label_term, float *s_out, int64_t ld_s,
                              float *g_emb_q, float *g_emb_db, float *grad_out,
                              float *loss_out, void *workspace, sg_stream_t stream);

/*
 * Backward of the node-level stack of `count` graphs (the arguments of sg_embed) from the
 * gradients of their embeddings, g_emb [count][E], E = sg_embed_dim(model): each wavefront
 * stages two graphs, reruns the forward of the stack with dropout off and runs its backward.
 * grad_out[0 .. head offset) = Σ over the count entries of ∂(g_emb[c] · embedding(c))/∂θ
 * (repeats in graph_idx allowed: the map is linear); the head's range is not touched.  The
 * head offset is the flat offset of the NTN's weights_W (n_params for the Dot head).
 * *status_out as in sg_embed: a bad id sets SG_ERR_ARG, a bad node count SG_ERR_SHAPE, and
 * that entry contributes nothing.  count == 0 zeroes the range.
 * NOT bitwise reproducible: the generic stack accumulates parameter gradients with LDS
 * float atomics, as the generic pair kernel does; results agree up to fp32 summation order.
 * workspace: sg_embed_bwd_workspace_bytes(model, count) bytes, -1 for a model the call does
 * not serve or a negative count.
 */
int64_t sg_embed_bwd_workspace_bytes(const sg_model_t *model, int64_t count);
int32_t sg_embed_bwd(const sg_model_t *model, const float *store_adj,
                     const int32_t *store_types, const int32_t *store_n, int32_t n_graphs,
                     int32_t n_max, const int32_t *graph_idx, int64_t count,
                     const float *params, const float *g_emb, float *grad_out,
                     int32_t *status_out, void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_EMBED_TRAIN_H */
