/*
 * siamese_web_embed.h — embed-once retrieval for graph-store (Web) models on
 * libsiamese_hip.so: graph-level embeddings from a CSR store and the m x n NTN score grid
 * at Padding / NTN widths D in [32, 512] (sg_model_validate path 3, BASELINE config C5).
 *
 * siamese_embed.h serves every other path; the factorisation is the same.  With dropout
 * off a graph's node stack (GCN -> GCN -> Dense -> Padding) does not depend on its partner,
 * and the NTN head (layers.py:282-310) factors per query,
 *   m_k(i, j) = [e_j, 1] · Q_i[:, k],
 *   Q_i[b][k] = Σ_a e_i[a] W[a][b][k] + V[k][D + b]  (b < D),
 *   Q_i[D][k] = V[k][:D] · e_i + bias[k],
 * so m queries against n database graphs need m + n runs of the node stack, one table of
 * O(m·D²·K) work and 2 (D + 1) K FLOP per pair instead of 2 D² K.
 *
 * INFERENCE MODE, as in siamese_embed.h: every call reads model->keep_prob as 1 (no
 * dropout in any layer, the head included), so an embedding depends on no seed or pair.
 *
 * Conventions are those of siamese_hip.h: caller-owned DEVICE buffers unless noted,
 * stream-ordered calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code.
 * Every entry point checks its arguments on the host before its first HIP call.  The
 * symbols are detected by presence: sg_version() does not change with them.
 */
#ifndef SIAMESE_WEB_EMBED_H
#define SIAMESE_WEB_EMBED_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Width D of one graph embedding (the Padding / NTN width) of a path-3 model.  Host-only.
 * -1 for NULL, an invalid model and every other path. */
int32_t sg_web_embed_dim(const sg_model_t *model);

/* Row stride of the embeddings sg_web_embed writes: D rounded up to a multiple of 128.
 * -1 as above. */
int32_t sg_web_embed_ld(const sg_model_t *model);

/*
 * Graph-level embeddings of `count` graphs of a CSR store (sg_csr_store_t, siamese_hip.h).
 * graph_idx [count] selects store graphs (repeats allowed), NULL = graphs 0 .. count-1.
 * emb_out [count][ld], ld = sg_web_embed_ld(model): columns [0, n_g) hold the node stack's
 * output of graph g (one value per node), columns [n_g, D) the Padding layer's
 * padding_value, columns [D, ld) zero; all ld columns are written.  A graph's row does not
 * depend on its position in the call or on the other graphs of the call.
 * *status_out (device int, may be NULL): an id outside the store sets SG_ERR_ARG, a node
 * count outside [1, store->n_max] SG_ERR_SHAPE; either way that row is written as zeros
 * and the other rows are unaffected.
 * Host checks as sg_web_forward: the store's pointers, store->n_max <= D and <=
 * model->n_max, the instance kernel's LDS.  count == 0 is SG_OK with no launch.
 * workspace: sg_web_embed_workspace_bytes(model, count) bytes, -1 for a model off path 3.
 */
int64_t sg_web_embed_workspace_bytes(const sg_model_t *model, int64_t count);
int32_t sg_web_embed(const sg_model_t *model, const sg_csr_store_t *store,
                     const int32_t *graph_idx, int64_t count, const float *params,
                     float *emb_out, int32_t *status_out, void *workspace, sg_stream_t stream);

/*
 * Score grid of the NTN head over embeddings: out[i * ld_out + j] = score of (query i as
 * graph 1, database j as graph 2).  emb_q [m] rows of stride ld_q, emb_db [n] rows of
 * stride ld_db; any stride >= D is accepted and only columns < D are read, so the strided
 * rows of sg_web_embed and a contiguous [n][D] array (D need not be a multiple of 4) both
 * serve.  apply_final = 0 gives the pre-activation score of sg_web_forward, apply_final = 1
 * applies model->final_act on the device.  Columns j >= n of a row of `out` are not written.
 * Serves every path-3 model (K in [1, 16], both ntn_modes, bias on or off, every
 * final_act); everything else gives SG_ERR_UNSUPPORTED.  m == 0 or n == 0 is SG_OK with
 * no launch.  Exact f32; results are bitwise reproducible.
 * workspace: sg_web_score_grid_workspace_bytes(model, m) bytes (the per-query tables Q_i),
 * -1 for a model the grid does not serve.
 */
int64_t sg_web_score_grid_workspace_bytes(const sg_model_t *model, int64_t m);
int32_t sg_web_score_grid(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                          const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                          const float *params, int32_t apply_final, float *out, int64_t ld_out,
                          void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_WEB_EMBED_H */
