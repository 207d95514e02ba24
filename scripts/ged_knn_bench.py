"""The k nearest graphs under exact GED (include/siamese_ged_knn.h) on the AIDS700nef-shaped
test x train grid (GPU only).

    python scripts/ged_knn_bench.py [--repeats 5] [--k 10] [--budget 1048576] [--out FILE.json]

One grid: the 140 test graphs of syn_aids700nef (the synthetic set of AIDS700nef's size
distribution; the repository ships no AIDS700nef files) against its 560 training graphs, 78,400
pairs of 5 .. 10 nodes, capacity 10, k = 10, the default budget of 2^20 expansions per pair.

  knn       one sg_ged_knn call (five launches) with candidates_out and expansions_out
  baseline  what the same answer cost before: one sg_ged_exact_grid call over the whole grid
            with lb_out and expansions_out, then a stable sort of every row by distance and
            its first k columns (torch.sort on the device)

Device times are HIP events around each with every output buffer allocated beforehand (the
sort writes into preallocated tensors; what it needs besides comes from torch's caching
allocator), after one warm-up of each; the repeats alternate between the two so a drift of the clocks falls on both;
median with min .. max.  Before timing, the certified rows must equal the baseline's top-k
wherever the baseline proved the whole row.

Four values are recorded, none of them a target: the candidate share (pairs that survived the
filter / all pairs), the expansion ratio (knn's expansions / the baseline's), the certified-row
share and the wall-time ratio (knn's median / the baseline's median).  Prints one JSON line.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


class Grid(object):
    """The test x train grid with the buffers of both routes; knn() and baseline() are the
    bare calls."""

    def __init__(self, store, q, db, k, budget, device):
        import torch
        from graphembedding_amd import _lib
        self._lib, self.store, self.k, self.budget = _lib, store, k, budget
        self.dev = store.to_device(device)
        i32 = dict(dtype=torch.int32, device=device)
        self.q, self.db = torch.as_tensor(q, **i32), torch.as_tensor(db, **i32)
        self.m, self.n = m, n = len(q), len(db)
        self.ws_knn = torch.empty(_lib.ged_knn_workspace_bytes(m, n, store.n_max, k) // 8 + 1,
                                  dtype=torch.int64, device=device)
        self.cols = torch.empty((m, k), **i32)
        self.kub = torch.empty((m, k), **i32)
        self.klb = torch.empty((m, k), **i32)
        self.cert = torch.empty((m,), **i32)
        self.cand = torch.empty((m,), **i32)
        self.kex = torch.empty((m,), dtype=torch.int64, device=device)
        self.ws = torch.empty(_lib.ged_exact_grid_workspace_bytes(m, n, store.n_max) // 4 + 1,
                              **i32)
        self.ub = torch.empty((m, n), **i32)
        self.lb = torch.empty((m, n), **i32)
        self.ex = torch.empty((m, n), dtype=torch.int64, device=device)
        self.status = torch.zeros(1, **i32)
        self.sorted = torch.empty((m, n), **i32)
        self.order = torch.empty((m, n), dtype=torch.int64, device=device)

    def knn(self):
        self._lib.ged_knn(self.dev, self.store.n_max, self.q, self.m, self.db, self.n, self.k,
                          self.budget, self.cols, self.kub, self.klb, self.cert, self.cand,
                          self.kex, self.status, self.ws_knn)

    def baseline(self):
        import torch
        self._lib.ged_exact_grid(self.dev, self.store.n_max, self.q, self.m, self.db, self.n,
                                 self.budget, self.ub, self.n, self.lb, None, self.ex,
                                 self.status, self.ws)
        torch.sort(self.ub, dim=1, stable=True, out=(self.sorted, self.order))

    def timed(self, fn):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


def _stats(ms):
    ms = sorted(ms)
    return dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], repeats=len(ms))


def main():
    import torch
    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.build import build_hip
    from graphembedding_amd.data import synthetic_graphs
    from graphembedding_amd.ged import GED_EXACT_DEFAULT_BUDGET
    build_hip()
    device = torch.device('cuda:0')
    repeats, k = _arg('--repeats', 5), _arg('--k', 10)
    budget = _arg('--budget', GED_EXACT_DEFAULT_BUDGET)
    store = load_graph_set('syn_aids700nef').store       # training graphs first, then test
    n_train = len(synthetic_graphs('syn_aids700nef', 123)[0])
    q, db = np.arange(n_train, len(store)), np.arange(n_train)
    g = Grid(store, q, db, k, budget, device)
    g.knn()   # warm-up
    g.baseline()
    torch.cuda.synchronize()
    assert int(g.status.item()) == 0
    cols, cert = g.cols.cpu().numpy(), g.cert.cpu().numpy().astype(bool)
    cand, kex = g.cand.cpu().numpy(), g.kex.cpu().numpy()
    ub, lb, ex = (t.cpu().numpy() for t in (g.ub, g.lb, g.ex))
    whole = (ub == lb).all(axis=1)                       # rows the baseline proved entirely
    top = g.order[:, :k].cpu().numpy()
    assert np.array_equal(cols[cert & whole], top[cert & whole])
    t_knn, t_base = [], []
    for _ in range(repeats):
        t_knn.append(g.timed(g.knn))
        t_base.append(g.timed(g.baseline))
    assert np.array_equal(g.cols.cpu().numpy(), cols) and np.array_equal(g.kex.cpu().numpy(), kex)
    sk, sb = _stats(t_knn), _stats(t_base)
    n = np.asarray(store.n)
    result = dict(
        bench='ged_knn', gpu=torch.cuda.get_device_name(0), grid='syn_aids700nef test x train',
        queries=g.m, database=g.n, pairs=g.m * g.n, k=k, budget=budget, n_max=store.n_max,
        nodes_min=int(n.min()), nodes_max=int(n.max()),
        knn=sk, baseline_exact_grid_and_sort=sb,
        candidate_share=float(cand.sum() / (g.m * g.n)),
        expansion_ratio=float(kex.sum() / max(int(ex.sum()), 1)),
        certified_row_share=float(cert.mean()),
        wall_time_ratio=float(sk['ms_median'] / sb['ms_median']),
        candidates=int(cand.sum()), candidates_per_row_min=int(cand.min()),
        candidates_per_row_max=int(cand.max()),
        knn_expansions=int(kex.sum()), baseline_expansions=int(ex.sum()),
        baseline_rows_proven_entirely=int(whole.sum()),
        certified_rows_checked_against_baseline=int((cert & whole).sum()))
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
