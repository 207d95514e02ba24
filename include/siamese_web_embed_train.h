/*
 * siamese_web_embed_train.h — embed-once training for graph-store (Web) models on
 * libsiamese_hip.so: the adjoint of the m x n NTN score grid at Padding / NTN widths
 * D in [32, 512] and the backward of the CSR node stack of single graphs
 * (sg_model_validate path 3, BASELINE config C5).
 *
 * siamese_embed_train.h serves every other path; the factorisation is the same.  With
 * dropout off a graph's node stack does not depend on its partner and the NTN head factors
 * per query (siamese_web_embed.h), so the loss of an m x n block of pairs needs
 *     sg_web_embed (siamese_web_embed.h)  →  sg_web_score_grid_fwd_bwd  →  [sum the
 *     query-role and database-role embedding gradients of each graph]  →  sg_web_embed_bwd
 * and leaves the same Σ ∂loss/∂θ in grad_out as sg_fwd_bwd over the m·n pairs (head range
 * from the grid call, node-layer range from sg_web_embed_bwd), up to fp32 summation order.
 *
 * DROPOUT 0 ONLY, as siamese_embed_train.h and for the same reason (the reference draws
 * its masks per pair, quirk A4): both calls and both workspace queries REFUSE
 * (SG_ERR_UNSUPPORTED, -1) a model in which a layer with dropout != 0 meets a
 * model->keep_prob whose keep threshold is not "keep all".
 *
 * Conventions are those of siamese_hip.h: caller-owned DEVICE buffers unless noted,
 * stream-ordered calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code.
 * Every entry point checks its arguments on the host before its first HIP call.  The
 * symbols are detected by presence: sg_version() does not change with them.
 */
#ifndef SIAMESE_WEB_EMBED_TRAIN_H
#define SIAMESE_WEB_EMBED_TRAIN_H

#include "siamese_web_embed.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Forward, loss and backward of the NTN head over the grid of (query i as graph 1,
 * database j as graph 2): sg_score_grid_fwd_bwd's contract (siamese_embed_train.h) on the
 * embeddings of sg_web_embed.
 *   emb_q [m] rows of stride ld_q, emb_db [n] rows of stride ld_db: any stride >= D, only
 *     columns < D are read (as sg_web_score_grid).
 *   labels [m][ld_labels] (ld_labels >= n): read by the aligned loss only (may be NULL for
 *     the broadcast loss).  batch_total, y_stats, add_label_term: as in sg_fwd_bwd; the
 *     sums run over the m·n pairs of this call.
 *   s_out [m][ld_s] (ld_s >= n; may be NULL): pre-activation scores, bitwise those of
 *     sg_web_score_grid(apply_final = 0); columns j >= n of a row are not written.
 *   g_emb_q [m] rows of stride ld_gq, g_emb_db [n] rows of stride ld_gdb (both >= D):
 *     ∂loss/∂embedding; columns < D are written, columns [D, ld) are left untouched.
 *   grad_out [n_params]: only the head's range (weights_W, weights_V, weights_U, bias: from
 *     the offset of weights_W to n_params) is written; the node-layer range in front of it
 *     is not touched (sg_web_embed_bwd writes it).
 *   loss_out [1] (may be NULL).
 * Serves every path-3 model without effective dropout (K in [1, 16], both ntn_modes, bias
 * on or off, every final_act, both loss modes).  Every model sg_web_score_grid refuses is
 * refused with the same code, model first; then dropout, then m or n above 2^29
 * (SG_ERR_UNSUPPORTED), then m == 0 or n == 0 (SG_OK, nothing written), then the pointers
 * and strides (SG_ERR_ARG).
 * Exact f32 (v_mfma_f32_16x16x4_f32), no float atomics: every sum across workgroups runs in
 * a fixed order and the launch shapes depend on (m, n, D, K) only, so two calls on equal
 * inputs give bitwise equal outputs.
 * workspace: sg_web_score_grid_bwd_workspace_bytes(model, m, n) bytes, -1 for a model the
 * call refuses, for negative m or n and for m or n above 2^29.  With Dq = D + 1 rounded up
 * to 4, n64 = n rounded up to 64 and up64(x) = x rounded up to 64:
 *   4 · ( 2 · up64(m · Dq · 16)                                 the tables Q_i and gQ_i
 *       + up64(min(min(m, 256) · n64 · 16, max(2^23, n64 · 16)))   GM of one query chunk
 *       + up64((n64 / 64 + 512) · 32) )                         workgroup partials: gU, loss
 *   + 256.
 * The grid is walked in chunks of qc = clamp(2^23 / (n64 · 16), 1, 256) queries whose
 * ∂loss/∂m_k, GM [qc][n64][16], is the only term proportional to pairs: at most 32 MiB
 * (or one query's n64 · 64 bytes, if larger).  No term is proportional to m·n·D.
 */
int64_t sg_web_score_grid_bwd_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n);
int32_t sg_web_score_grid_fwd_bwd(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                                  const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                                  const float *params, const float *labels, int64_t ld_labels,
                                  int64_t batch_total, const float *y_stats,
                                  int32_t add_label_term, float *s_out, int64_t ld_s,
                                  float *g_emb_q, int64_t ld_gq, float *g_emb_db,
                                  int64_t ld_gdb, float *grad_out, float *loss_out,
                                  void *workspace, sg_stream_t stream);

/*
 * Backward of the node stack of `count` graphs of a CSR store (the arguments of
 * sg_web_embed) from the gradients of their embeddings, g_emb [count] rows of stride ld_g
 * (ld_g >= D; only the columns below a graph's node count matter, the Padding columns are
 * constants):
 *   grad_out[0 .. offset of weights_W) = Σ over the count entries of
 *   ∂(g_emb[c] · embedding(c))/∂θ
 * (repeats in graph_idx allowed: the map is linear; NULL = graphs 0 .. count-1); the head's
 * range is not touched.  *status_out as in sg_web_embed: a bad id sets SG_ERR_ARG, a bad
 * node count SG_ERR_SHAPE, and that entry contributes nothing.  count == 0 zeroes the range.
 * Host checks are sg_web_embed's plus the dropout refusal above.
 * The entries run in chunks of cc = min(count, 1024): the forward instance kernel stores
 * each chunk's keep bits and D2 rows, the backward instance kernel of the pair path reads
 * them and adds into one gradient row per workgroup, chunk after chunk in stream order;
 * one fixed-order column sum follows.  Two calls on one device agree bitwise.
 * workspace: sg_web_embed_bwd_workspace_bytes(model, count) bytes, -1 for a model the call
 * refuses or a count outside [0, 2^29].  With Dp = sg_web_embed_ld(model), cc as above and
 * n_gcn the length of the node-layer range:
 *   4 · ( up64(512 · n_gcn)        gradient rows (a device with more than 512 CUs is refused)
 *       + 2 · up64(cc · Dp)        the chunk's embeddings and its rows of g_emb
 *       + up64(cc · Dp · 4)        keep bits, uint16 [2 cc][Dp][4]
 *       + up64(cc · Dp · 32)       D2 rows [2 cc][Dp][16]
 *       + up64(cc)                 the chunk's graph ids
 *       + sg_web_embed_workspace_bytes(model, cc) / 4 )   instance records and unit sort
 *   + 256.
 */
int64_t sg_web_embed_bwd_workspace_bytes(const sg_model_t *model, int64_t count);
int32_t sg_web_embed_bwd(const sg_model_t *model, const sg_csr_store_t *store,
                         const int32_t *graph_idx, int64_t count, const float *params,
                         const float *g_emb, int64_t ld_g, float *grad_out,
                         int32_t *status_out, void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_WEB_EMBED_TRAIN_H */
