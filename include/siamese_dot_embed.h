/*
 * siamese_dot_embed.h — embed-once retrieval, search and training for models whose pair head
 * is Dot (layers.py:230-252) on libsiamese_hip.so: the m x n score grid, the fused score
 * grid + per-row top-k, and the grid's forward + loss + adjoint.
 *
 * The Dot head of (query i as graph 1, database j as graph 2) is  s(i, j) = Σ_a e_i[a]·e_j[a]
 * over the E = sg_embed_dim(model) components of the two graph embeddings.  It has no
 * variables, no dropout of its own and no per-query table: the score matrix is E_q · E_dbᵀ and
 * its adjoint is two more matrix products.  The embeddings come from sg_embed (siamese_embed.h)
 * or sg_embed_drop (siamese_embed_drop.h), their gradients go back through sg_embed_bwd
 * (siamese_embed_train.h) or sg_embed_drop_bwd; those calls serve Dot models already (the head
 * offset of a Dot model is n_params, so the node-stack backward writes the whole gradient).
 * The NTN calls of siamese_embed.h, siamese_search.h and siamese_embed_train.h keep refusing
 * the Dot head; the calls here refuse every other head.
 *
 * Models served: pair head Dot, sg_model_validate path 0, 1 or 2, 1 <= E <= 512.  Anything
 * else (the NTN head, the graph-store path 3, E > 512) gives SG_ERR_UNSUPPORTED and -1 from
 * the workspace queries.  Normalised (cosine) scores are not offered.
 *
 * THE ARITHMETIC OF ONE SCORE — the contract of every call here.  s(i, j) is one accumulator
 * chain of v_mfma_f32_16x16x4_f32, starting from 0: k-step t = 0, 1, … ceil(E / 4) - 1 adds
 * the four products of components a = 4 t .. 4 t + 3, in ascending t; components a >= E of the
 * last k-step are zeros.  Query rows are always the A operand and database rows the B operand.
 * A score therefore does not depend on the launch shape, on m, on n, on the row strides or on
 * where its two rows sit in their arrays, and all three calls produce the same bits for the
 * same pair of rows.  With integer-valued embeddings whose partial sums stay below 2^24 every
 * step is exact.
 *
 * Conventions are those of siamese_embed.h: caller-owned DEVICE buffers, stream-ordered calls,
 * no allocation, no host synchronisation, SG_OK or an SG_ERR_* code, every argument checked on
 * the host, in the order stated with each call, before the first HIP call.  model->keep_prob
 * and model->adj_dtype are not read by the two inference calls.  Embeddings are rows of
 * stride ld_q / ld_db >= E floats; only columns < E are read.  The symbols' presence is how a
 * caller detects the feature; sg_version() does not change with them.
 */
#ifndef SIAMESE_DOT_EMBED_H
#define SIAMESE_DOT_EMBED_H

#include "siamese_embed.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * out[i * ld_out + j] = s(i, j), or sg_final(model->final_act, model->yeta, s(i, j))
 * (similarity.py:55-60) when apply_final != 0.  Columns j >= n of a row of `out` are not
 * written.  No params and no workspace: the head has no variables.
 * Refusals, in this order:
 *  1. model NULL, m < 0 or n < 0: SG_ERR_ARG;
 *  2. the model: an invalid model gives the code of its plan, a model this header does not
 *     serve SG_ERR_UNSUPPORTED;
 *  3. m or n above 2^29: SG_ERR_UNSUPPORTED;
 *  4. m == 0 or n == 0: SG_OK, nothing is written;
 *  5. a NULL emb_q, emb_db or out, ld_q < E, ld_db < E, ld_out < n: SG_ERR_ARG;
 *  6. more than 2^31 - 1 tiles of 64 x 64 scores: SG_ERR_UNSUPPORTED.
 */
int32_t sg_dot_score_grid(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                          const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                          int32_t apply_final, float *out, int64_t ld_out, sg_stream_t stream);

/*
 * idx_out [m][k] (database rows) and val_out [m][k] (their scores, may be NULL), best first:
 * bit for bit what sg_dot_score_grid(..., apply_final, out, ...) followed by
 * sg_topk_rows(out, m, n, ld, k, largest, ...) return (the same floats, the same total order:
 * by value, descending when largest != 0; ties to the smaller column; NaN after every number
 * and by column; -0 ranks with +0), without the m x n matrix.  The result depends neither on
 * seg_cols nor on the device.
 * Refusals, in this order:
 *  1. and 2. as sg_dot_score_grid;
 *  3. k < 1 SG_ERR_ARG, k > 64 SG_ERR_UNSUPPORTED, k > n SG_ERR_ARG (so n == 0 is an error
 *     here, as in sg_search_topk), seg_cols negative or not a multiple of 64 SG_ERR_ARG, m or
 *     n above 2^29 SG_ERR_UNSUPPORTED;
 *  4. m == 0: SG_OK, nothing is written;
 *  5. a NULL emb_q, emb_db, idx_out or workspace, a workspace that is not 8-byte aligned,
 *     ld_q < E, ld_db < E: SG_ERR_ARG.
 * seg_cols: the database columns one workgroup scans, a positive multiple of 64, or 0 for the
 * library's choice (it may depend on the device).  The database is cut into S =
 * ceil(n / seg_cols) segments; each leaves k candidates per query and sg_search_topk's merge
 * kernel picks the k best when S > 1.
 * workspace: sg_dot_search_topk_workspace_bytes(model, m, n, k, seg_cols) bytes, for the same
 * seg_cols as the call (-1 for what the call refuses under 1 to 3):
 *     S · m · k · 8  candidate keys  +  S · m · k · 4  candidate values  +  256.
 * With seg_cols = 0 the library picks 1024 <= seg_cols <= 65536 by m, k and the device, and
 * the workspace is that of the shortest choice, S = ceil(n / 1024), on every device: the size
 * is monotone in m, n and k.
 */
int64_t sg_dot_search_topk_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n,
                                           int32_t k, int64_t seg_cols);
int32_t sg_dot_search_topk(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                           const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                           int32_t apply_final, int32_t k, int32_t largest, int64_t seg_cols,
                           int32_t *idx_out, float *val_out, void *workspace,
                           sg_stream_t stream);

/*
 * Forward, loss and backward of the Dot head over the grid.
 *   labels [m][ld_labels] (ld_labels >= n): y of pair (i, j); read by the aligned loss only
 *     (may be NULL for the broadcast loss).
 *   batch_total, y_stats (device {ȳ, ½Σ(y−ȳ)²}), add_label_term: exactly as in
 *     sg_score_grid_fwd_bwd (siamese_embed_train.h).  With ŷ = sg_final(s): the broadcast loss
 *     is ½Σ(ŷ−ȳ)² (+ y_stats[1] when add_label_term) with gy = ŷ−ȳ, the aligned loss
 *     ½Σ(ŷ−y)²/batch_total with gy = (ŷ−y)/batch_total; the sums run over the m·n pairs.
 *   s_out [m][ld_s] (ld_s >= n; may be NULL): the pre-activation scores, bitwise those of
 *     sg_dot_score_grid with apply_final = 0; columns j >= n are not written.
 *   g_emb_q [m][E], g_emb_db [n][E] (dense rows of E floats): ∂loss/∂embedding,
 *     g_emb_q = GS · E_db and g_emb_db = GSᵀ · E_q with GS[i][j] = gy · sg_final'(s), both on
 *     v_mfma_f32_16x16x4_f32.  Rows past m and n are not touched.
 *   loss_out [1] (may be NULL).
 * There is no params and no grad_out argument: the head has no variables.
 * Refusals, in this order:
 *  1. and 2. as sg_dot_score_grid; then model->keep_prob outside (0, 1] SG_ERR_ARG, and any
 *     layer with an effective keep probability below 1 SG_ERR_UNSUPPORTED (dropout 0 only, as
 *     siamese_embed_train.h explains; under graph-keyed dropout the caller passes a copy of
 *     the model with keep_prob = 1, the masks being in the embeddings already);
 *  3. m or n above 2^29, a workspace beyond 2^60 bytes or a launch beyond 2^31 - 1
 *     workgroups: SG_ERR_UNSUPPORTED;
 *  4. m == 0 or n == 0: SG_OK, nothing is written;
 *  5. a NULL emb_q, emb_db, g_emb_q, g_emb_db or workspace, a workspace that is not 16-byte
 *     aligned, ld_q < E, ld_db < E, ld_labels < n, ld_s < n with s_out given, the broadcast
 *     loss without y_stats, the aligned loss without labels or with batch_total <= 0:
 *     SG_ERR_ARG.
 * Deterministic: no float atomics; the launch shape is a function of (m, n, E) alone, each
 * workgroup's loss partial and each partial product are summed in a fixed order, so two calls
 * on equal inputs give bitwise equal outputs, on every device.
 * workspace: sg_dot_score_grid_bwd_workspace_bytes(model, m, n) bytes; -1 for what the call
 * refuses under 1 to 3.  With up64(x) = x rounded up to 64, T(x) = ceil(x / 64) and
 * C(x) = ceil(x / 512), in floats:
 *     up64(m · n)               GS [m][n]
 *   + up64(T(m) · T(n))         one loss partial per 64 x 64 tile
 *   + up64(C(n) · m · E)        partial products of g_emb_q, one per 512 database rows
 *   + up64(C(m) · n · E)        partial products of g_emb_db, one per 512 queries
 * times 4, plus 256 bytes: monotone in m and n, the same on every device.
 */
int64_t sg_dot_score_grid_bwd_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n);
int32_t sg_dot_score_grid_fwd_bwd(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                                  const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                                  const float *labels, int64_t ld_labels, int64_t batch_total,
                                  const float *y_stats, int32_t add_label_term, float *s_out,
                                  int64_t ld_s, float *g_emb_q, float *g_emb_db,
                                  float *loss_out, void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_DOT_EMBED_H */
