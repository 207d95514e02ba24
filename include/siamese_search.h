/*
 * siamese_search.h — embed-once search on libsiamese_hip.so: the k best database graphs of
 * every query straight from the embeddings, without the m x n score matrix.
 *
 * sg_score_grid followed by sg_topk_rows (siamese_embed.h) writes m·n scores and reads
 * them k times; a search over a large index needs neither.  sg_search_topk computes the
 * same scores tile by tile and keeps a running top-k per query on the chip, so its memory
 * is the per-query tables plus a few candidate lists, and none of it grows with m·n.
 *
 * Conventions are those of siamese_embed.h: caller-owned DEVICE buffers, stream-ordered
 * calls, no allocation, no host synchronisation, SG_OK or an SG_ERR_* code, arguments
 * checked on the host before the first HIP call, INFERENCE MODE (model->keep_prob is read
 * as 1).  The symbols' presence is how a caller detects the feature; sg_version() does not
 * change with them.
 */
#ifndef SIAMESE_SEARCH_H
#define SIAMESE_SEARCH_H

#include "siamese_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * idx_out [m][k] (database rows) and val_out [m][k] (their scores, may be NULL), best
 * first, of (query i as graph 1, database j as graph 2) over emb_q [m][D], emb_db [n][D].
 * Both equal, bit for bit, what sg_score_grid(model, emb_q, emb_db, m, n, params,
 * apply_final, out, ...) followed by sg_topk_rows(out, m, n, ld, k, largest, ...) return:
 * the same float scores and the same total order (by value, descending when largest != 0;
 * ties to the smaller column; NaN after every number and by column; -0 ranks with +0).
 *
 * Serves the models sg_score_grid serves (the NTN head with D <= 31 and feature_map_dim
 * <= 16, both ntn_modes, every inneract, bias on or off); every other model gives
 * SG_ERR_UNSUPPORTED and a workspace of -1.
 * 1 <= k <= min(n, 64): k > 64 gives SG_ERR_UNSUPPORTED, k < 1 or k > n SG_ERR_ARG.
 * m, n <= 2^29 (SG_ERR_UNSUPPORTED above).  m == 0 returns SG_OK with no work.
 *
 * seg_cols: the database columns one workgroup scans, a positive multiple of 64, or 0 for
 * the library's choice (it may depend on the device); anything else gives SG_ERR_ARG.  The
 * database is cut into S = ceil(n / seg_cols) segments; each leaves k candidates per query
 * and a second kernel merges them when S > 1.  The result does not depend on seg_cols (the
 * selection is exact over a total order); smaller segments give more parallelism and a
 * larger workspace.
 *
 * workspace: sg_search_topk_workspace_bytes(model, m, n, k, seg_cols) bytes, for the same
 * seg_cols as the call (-1 for a model or arguments the call refuses):
 *     align256(m · Dp · 16 · 4)        the query tables Q [m][Dp][16], Dp = (D + 4) & ~3
 *   + S · m · k · 8                    candidate keys [S][m][k]
 *   + S · m · k · 4                    candidate values [S][m][k]
 *   + 256
 * With seg_cols = 0 the library picks 1024 <= seg_cols <= 65536 by m, k and the device, and
 * the workspace is that of the shortest choice, S = ceil(n / 1024), on every device.
 */
int64_t sg_search_topk_workspace_bytes(const sg_model_t *model, int64_t m, int64_t n,
                                       int32_t k, int64_t seg_cols);
int32_t sg_search_topk(const sg_model_t *model, const float *emb_q, const float *emb_db,
                       int64_t m, int64_t n, const float *params, int32_t apply_final,
                       int32_t k, int32_t largest, int64_t seg_cols, int32_t *idx_out,
                       float *val_out, void *workspace, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIAMESE_SEARCH_H */
