/*
 * siamese_web_search.h — embed-once search for graph-store (Web) models on
 * libsiamese_hip.so: the k best database graphs of every query straight from the
 * embeddings of sg_web_embed (siamese_web_embed.h), without the m x n score matrix.
 *
 * sg_web_score_grid followed by sg_topk_rows (siamese_embed.h) writes m·n scores and reads
 * them k times.  Graph-store models are the ones with the largest databases, so an index too
 * large for that matrix is their normal case.  sg_web_search_topk computes the same scores
 * tile by tile and keeps a running top-k per query on the chip: its memory is the per-query
 * tables plus a few candidate lists, and none of it grows with m·n.  siamese_search.h is the
 * same call for every other path (D <= 31); it keeps refusing graph-store models.
 *
 * Conventions are those of siamese_search.h and siamese_web_embed.h: caller-owned DEVICE
 * buffers, stream-ordered calls, no allocation, no host synchronisation, SG_OK or an
 * SG_ERR_* code, arguments checked on the host before the first HIP call, INFERENCE MODE
 * (model->keep_prob is read as 1).  The symbols' presence is how a caller detects the
 * feature; sg_version() does not change with them.
 */
#ifndef SIAMESE_WEB_SEARCH_H
#define SIAMESE_WEB_SEARCH_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * idx_out [m][k] (database rows) and val_out [m][k] (their scores, may be NULL), best
 * first, of (query i as graph 1, database j as graph 2) over emb_q [m] rows of stride ld_q
 * and emb_db [n] rows of stride ld_db (any stride >= D; only columns < D are read, so the
 * strided rows of sg_web_embed and a contiguous [n][D] array both serve).
 * Both equal, bit for bit, what sg_web_score_grid(model, emb_q, ld_q, emb_db, ld_db, m, n,
 * params, apply_final, out, ...) followed by sg_topk_rows(out, m, n, ld, k, largest, ...)
 * return: the same float scores and the same total order (by value, descending when
 * largest != 0; ties to the smaller column; NaN after every number and by column; -0 ranks
 * with +0).  The result depends neither on seg_cols nor on the device.
 *
 * Refusals, in this order:
 *  1. the model, as sg_web_score_grid: NULL gives SG_ERR_ARG, a model off path 3 the code of
 *     its head plan (SG_ERR_UNSUPPORTED for a valid model of another path), feature_map_dim
 *     > 16 SG_ERR_UNSUPPORTED;
 *  2. k, seg_cols, m and n, as sg_search_topk: k < 1 SG_ERR_ARG, k > 64 SG_ERR_UNSUPPORTED,
 *     k > n SG_ERR_ARG, seg_cols negative or not a multiple of 64 SG_ERR_ARG, m or n above
 *     2^29 SG_ERR_UNSUPPORTED (negative: SG_ERR_ARG, with the model); m == 0 then returns
 *     SG_OK with no work;
 *  3. a NULL emb_q, emb_db, params, idx_out or workspace, ld_q < D, ld_db < D: SG_ERR_ARG.
 *
 * seg_cols: the database columns one workgroup scans, a positive multiple of 64, or 0 for
 * the library's choice (it may depend on the device).  The database is cut into S =
 * ceil(n / seg_cols) segments; each leaves k candidates per query and a second kernel
 * merges them when S > 1.  Smaller segments give more parallelism and a larger workspace.
 *
 * workspace: sg_web_search_topk_workspace_bytes(model, m, n, k, seg_cols) bytes, for the
 * same seg_cols as the call (-1 for a model or arguments the call refuses under 1 or 2):
 *     align256(m · Dq · 16 · 4)        the query tables Q [m][Dq][16], Dq = (D + 4) & ~3
 *   + S · m · k · 8                    candidate keys [S][m][k]
 *   + S · m · k · 4                    candidate values [S][m][k]
 *   + 256                              of which up to 15 bytes move the tables to the first
 *                                      16-byte boundary of the workspace
 * With seg_cols = 0 the library picks 1024 <= seg_cols <= 65536 by m, k and the device, and
 * the workspace is that of the shortest choice, S = ceil(n / 1024), on every device: the
 * size is monotone in m and in k.
 */
int64_t sg_web_search_topk_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n,
                                           int32_t k, int64_t seg_cols);
int32_t sg_web_search_topk(const sg_model_t *model, const float *emb_q, int64_t ld_q,
                           const float *emb_db, int64_t ld_db, int64_t m, int64_t n,
                           const float *params, int32_t apply_final, int32_t k, int32_t largest,
                           int64_t seg_cols, int32_t *idx_out, float *val_out,
                           void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_WEB_SEARCH_H */
