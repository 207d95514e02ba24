/*
 * siamese_embed.h — embed-once retrieval on libsiamese_hip.so (library 1.10): graph-level
 * embeddings, the m x n NTN score grid and per-row top-k.
 *
 * The reference scores its test matrix with one sess.run per (test i, train j) pair
 * (model/Siamese/train.py:47-74), which runs the whole GCN stack of both graphs for every
 * pair.  The model is Siamese (models.py:39-65, model_mse.py:104-129): with dropout off a
 * graph's node stack does not depend on its partner, and the NTN head (layers.py:282-310)
 * factors per query,  m_k(i, j) = [e_j, 1] · Q_i[:, k].  So n database graphs and m queries
 * need m + n runs of the node stack and one batched small-k GEMM.
 *
 * INFERENCE MODE — a deliberate deviation from the reference, which leaves dropout on in
 * its test runs (quirk A4): every call here reads model->keep_prob as 1 (no dropout in
 * any layer, the head included) and ignores model->adj_dtype (the dense f32 graph store of
 * sg_pack_pairs is read).  An embedding therefore does not depend on a seed or a pair.
 *
 * Conventions are those of siamese_hip.h: caller-owned DEVICE buffers unless noted,
 * stream-ordered calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code.
 * Every entry point checks its arguments on the host before its first HIP call.
 * Models on the graph-store path (sg_model_validate path 3) are not served here.
 */
#ifndef SIAMESE_EMBED_H
#define SIAMESE_EMBED_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Width E of the head's per-graph input (what NTN / Dot consume, layers.py:249, 282):
 * Padding max_in_dims x the width entering it for the default stack, the GCN width for
 * Average / Attention pooling.  Host-only.  -1 for an invalid model and for path 3.
 */
int32_t sg_embed_dim(const sg_model_t *model);

/*
 * Graph-level embeddings: the node-level stack of models.py:39-65 (layers.py:91-227) up
 * to the pair head, for `count` graphs of a dense-slot store (sg_pack_pairs' store_adj
 * [n_graphs][n_max][n_max], store_types [n_graphs][n_max], store_n [n_graphs]; n_max must
 * equal model->n_max).  graph_idx [count] selects store graphs (repeats allowed), NULL =
 * graphs 0 .. count-1.  emb_out [count][E], E = sg_embed_dim(model).
 * *status_out (device int, may be NULL): an id outside the store sets SG_ERR_ARG, a node
 * count outside [1, min(n_max, Padding max_in_dims)] (tf.pad, layers.py:226, quirk A9)
 * sets SG_ERR_SHAPE; either way that graph's row is written as zeros.
 */
int32_t sg_embed(const sg_model_t *model, const float *store_adj, const int32_t *store_types,
                 const int32_t *store_n, int32_t n_graphs, int32_t n_max,
                 const int32_t *graph_idx, int64_t count, const float *params,
                 float *emb_out, int32_t *status_out, sg_stream_t stream);

/*
 * Score grid of the NTN head (layers.py:282-310) over embeddings: out[i * ld_out + j] =
 * score of (query i as graph 1, database j as graph 2), emb_q [m][D], emb_db [n][D], D =
 * the NTN input_dim.  apply_final = 0 gives the pre-activation s of sg_forward
 * (pred_sim_without_act, models.py:90-91); apply_final = 1 applies model->final_act
 * (similarity.py:55-60) on the device.  Columns j >= n of a row of `out` are not written.
 * Serves the NTN head with D <= 31 and feature_map_dim <= 16, both ntn_modes, every
 * inneract, bias on or off; the Dot head, larger heads and path 3 give SG_ERR_UNSUPPORTED.
 * workspace: sg_score_grid_workspace_bytes(model, m) bytes (the per-query tables Q_i),
 * -1 for a model the grid does not serve.
 */
int64_t sg_score_grid_workspace_bytes(const sg_model_t *model, int64_t m);
int32_t sg_score_grid(const sg_model_t *model, const float *emb_q, const float *emb_db,
                      int64_t m, int64_t n, const float *params, int32_t apply_final,
                      float *out, int64_t ld_out, void *workspace, sg_stream_t stream);

/*
 * The k best entries of each row of vals [m] rows of n, row stride ld: idx_out [m][k]
 * columns and val_out [m][k] values (may be NULL), best first: the first k entries of a
 * row of the reference's sort_id_mat (src/results.py:221-224, read by top_k_ids,
 * results.py:51-72).  The order is total: by value (descending when largest != 0, else
 * ascending), ties to the smaller column (the reference's reversed stable argsort puts the
 * larger column of a tie first), NaN after every number (±inf included), NaNs by column.
 * vals is not modified.
 * 1 <= k <= min(n, 64): k > 64 gives SG_ERR_UNSUPPORTED, k < 1 or k > n SG_ERR_ARG.
 */
int32_t sg_topk_rows(const float *vals, int64_t m, int64_t n, int64_t ld, int32_t k,
                     int32_t largest, int32_t *idx_out, float *val_out, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_EMBED_H */
