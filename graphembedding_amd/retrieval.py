"""Embed-once retrieval over a trained Siamese model (include/siamese_embed.h).

The reference ranks a query against the database with one `sess.run` per (query,
database) pair (model/Siamese/train.py:47-74).  An EmbeddingIndex runs the node stack of
every database graph once, keeps the graph-level embeddings on the device, and scores
queries against all of them with the NTN score-grid kernel; `topk` returns the most
similar database graphs.  Inference mode: dropout is off (the reference leaves it on in
its test runs, quirk A4), so an index is reproducible and independent of any seed.
"""
from __future__ import annotations

from typing import Sequence

from .packer import GraphStore


class EmbeddingIndex(object):
    def __init__(self, model, graphs: Sequence):
        """model: SiameseGCNTNMSE; graphs: ModelGraphs.  A graph-store (Web) model embeds
        from a CSR store and scores with the large-D grid (include/siamese_web_embed.h)."""
        self.model = model
        self.n = len(graphs)
        self.embeddings = self._embed(graphs)       # torch float32 [n][embed_dim], device

    def _embed(self, graphs: Sequence):
        m = self.model
        if m.is_web:
            from .web import CsrStore
            return m.web_embed(CsrStore(list(graphs), m.input_dim, m.n_max))
        return m.embed(GraphStore(list(graphs), m.n_max, m.input_dim))

    def scores(self, query_graphs: Sequence, final: bool = True):
        """Similarity matrix [m][n] (torch, device): row i = query i as graph 1 against
        every indexed graph as graph 2; final=False gives the pre-activation scores."""
        grid = self.model.web_score_grid if self.model.is_web else self.model.score_grid
        return grid(self._embed(query_graphs), self.embeddings, final=final)

    def topk(self, query_graphs: Sequence, k: int, largest: bool = True):
        """(idx int32 [m][k], sims [m][k]): the k most similar indexed graphs per query,
        best first, ties to the smaller index."""
        return self.model.topk(self.scores(query_graphs), k, largest=largest)

    def search(self, query_graphs: Sequence, k: int, largest: bool = True):
        """What topk returns, from one fused call that keeps a running top-k per query on
        the chip and never holds the [m][n] similarity matrix (include/siamese_search.h):
        the way to query an index too large for `scores`.  Not for graph-store (Web) models:
        use `nearest`, which runs the fused search of either kind of model."""
        if self.model.is_web:
            from ._lib import SiameseHipError
            raise SiameseHipError('EmbeddingIndex.search: graph-store (Web) models are served '
                                  'by nearest (fused) or topk')
        return self.model.search(self._embed(query_graphs), self.embeddings, k, largest=largest)

    def nearest(self, query_graphs: Sequence, k: int, largest: bool = True):
        """What topk returns, bit for bit, from the fused search of the model's kind:
        web_search on a graph-store (Web) model (include/siamese_web_search.h), search on
        every other (include/siamese_search.h).  Neither holds the [m][n] matrix."""
        fused = self.model.web_search if self.model.is_web else self.model.search
        return fused(self._embed(query_graphs), self.embeddings, k, largest=largest)
