"""Device-side evaluation of the test matrix (include/siamese_eval.h): ap@k, MRR and "mse"
from the float32 score matrix the grid calls leave in device memory, without the host's
repeated full-matrix sorts.

metrics.py's three metrics decompose per query row into small integer counts (hits per k,
best predicted rank of a true top-1 graph) and one float64 sum.  sg_eval_rows produces them
in one launch; the few floating-point operations that turn them into the metrics are done
here exactly as metrics.py does them, so equal integers give bit-equal ap@k and MRR.
"""
from __future__ import annotations

import numpy as np
from scipy.stats import hmean

from . import _lib

EVAL_KS = (1, 2, 5, 10, 20, 50, 100)   # Eval.eval_test's k's (those below n)


def true_ranks(dist_mat) -> np.ndarray:
    """tr[q][j] = #{j' : d[q][j'] < d[q][j]}, int32 [m][n], in float64.  Graph j is in the
    tie-inclusive true top-k of Result.top_k_ids(q, k, norm, inclusive=True) exactly when
    tr[q][j] < k: that set is every graph at most as far as the k-th nearest."""
    d = np.asarray(dist_mat, dtype=np.float64)
    m, n = d.shape
    order = np.argsort(d, axis=1, kind='mergesort')
    srt = np.take_along_axis(d, order, axis=1)
    # a sorted position's rank is the first position of its run of equal values (the same ==
    # top_k_ids compares neighbours with)
    first = np.zeros((m, n), dtype=np.int64)
    if n > 1:
        first[:, 1:] = np.where(srt[:, 1:] == srt[:, :-1], 0, np.arange(1, n))
    first = np.maximum.accumulate(first, axis=1)
    tr = np.empty((m, n), dtype=np.int32)
    np.put_along_axis(tr, order, first.astype(np.int32), axis=1)
    return tr


class TruthTable(object):
    """What sg_eval_rows needs of the ground truth, for norm=True and norm=False: the true
    tie-best ranks, the float64 true similarities and the k's Eval.eval_test would use.
    Built on the host once (the ground truth never changes) and uploaded once."""

    def __init__(self, true_result, sim_kernel, yeta, device):
        import torch
        self.m, self.n = (int(x) for x in true_result.m_n())
        if self.n < 2:
            raise RuntimeError('device evaluation needs at least 2 database graphs (every k is '
                               'below n)')
        self.device = device
        self.ks = [k for k in EVAL_KS if k < self.n]
        self.ranks, self.sims = {}, {}
        for norm in (True, False):
            tr = true_ranks(true_result.dist_sim_mat(norm))
            sim = np.ascontiguousarray(true_result.sim_mat(sim_kernel, yeta, norm),
                                       dtype=np.float64)
            self.ranks[norm] = torch.from_numpy(tr).to(device)
            self.sims[norm] = torch.from_numpy(sim).to(device)


def eval_counts(scores, true_rank, true_sim, ks):
    """One sg_eval_rows call over a float32 device matrix [m][n] (unit column stride):
    (hits int32 [m][nk], best int32 [m], sqerr float64 [m] or None, nans int32 [m]) as
    device tensors."""
    import torch
    if scores.dtype != torch.float32 or scores.dim() != 2 or not scores.is_cuda:
        raise ValueError('scores: a float32 device matrix is expected')
    m, n = (int(x) for x in scores.shape)
    if n > 1 and scores.stride(1) != 1:
        scores = scores.contiguous()
    ld = int(scores.stride(0)) if m > 1 else n
    if ld < n:
        scores, ld = scores.contiguous(), n
    if tuple(true_rank.shape) != (m, n) or true_rank.dtype != torch.int32:
        raise ValueError('true_rank: int32 [{}][{}] expected'.format(m, n))
    true_rank = true_rank.contiguous()
    if true_sim is not None:
        if tuple(true_sim.shape) != (m, n) or true_sim.dtype != torch.float64:
            raise ValueError('true_sim: float64 [{}][{}] expected'.format(m, n))
        true_sim = true_sim.contiguous()
    dev = scores.device
    nbytes = _lib.eval_workspace_bytes(m, n, len(ks))
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dev) if nbytes else None
    hits = torch.empty((m, len(ks)), dtype=torch.int32, device=dev)
    best = torch.empty(m, dtype=torch.int32, device=dev)
    nans = torch.empty(m, dtype=torch.int32, device=dev)
    sqerr = torch.empty(m, dtype=torch.float64, device=dev) if true_sim is not None else None
    _lib.eval_rows(scores, m, n, ld, true_rank, true_sim, ks, hits, best, sqerr, nans, ws)
    return hits, best, sqerr, nans


def eval_rows(scores, truth, norm):
    """(aps, mrr, mse) of a float32 device score matrix against a TruthTable: what
    metrics.precision_at_ks (for truth.ks), mean_reciprocal_rank and mean_squared_error
    return for the same matrix cast to float64.  aps and mrr are bit-equal to the host's;
    mse differs by the summation order of m·n float64 squares."""
    m, n = truth.m, truth.n
    if tuple(scores.shape) != (m, n):
        raise ValueError('scores {} against a {}x{} ground truth'.format(tuple(scores.shape),
                                                                         m, n))
    hits, best, sqerr, nans = eval_counts(scores, truth.ranks[norm], truth.sims[norm], truth.ks)
    nans = nans.cpu().numpy()
    if nans.any():
        raise ValueError('NaN scores in {} of {} query rows (first: row {})'.format(
            int(np.count_nonzero(nans)), m, int(np.flatnonzero(nans)[0])))
    # metrics.py's arithmetic: len(truth & guess) / k per entry, then the mean over queries
    ps = hits.cpu().numpy().astype(np.float64) / np.asarray(truth.ks, dtype=np.float64)
    aps = np.mean(ps, axis=0)
    mrr = 1.0 / hmean(best.cpu().numpy().astype(np.float64))
    mse = np.sqrt(np.sum(sqerr.cpu().numpy())) / (m * n)
    return aps, mrr, mse
