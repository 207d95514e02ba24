"""The device GED bounds (include/siamese_ged.h) against a host solver (GPU only).

    python scripts/ged_bench.py [--repeats 7] [--sample 300] [--out FILE.json]

Two grids, each one sg_ged_grid call (two launches) with both_orders, lb_out and no map:
  aids700nef  syn_aids700nef, 700 x 700 = 490,000 pairs of 5 .. 10 nodes, capacity 10
  cap32       2,048 synthetic graphs of 5 .. 30 nodes (data.synthetic_graph), capacity 32,
              2,048 x 2,048 = 4,194,304 pairs
Device times are HIP events around the call with every buffer allocated beforehand, after one
warm-up call per grid; the repeats alternate between the grids (a, b, a, b, ...) so a drift of
the clocks falls on both; median with min .. max.  The `ub_only` rows time the same grids with
one assignment order and no lower bound (one of the three solves).
Host yardstick on --sample random pairs of the same grid, one process, one core:
  scipy        scipy.optimize.linear_sum_assignment on the three matrices of the pair plus
               the induced cost of both orders on the host (numpy)
  restatement  tests/_ged_restatement.py (the tie-exact specification, pure numpy)
as pairs/s, extrapolated to the grid.  Before timing, ub and lb of the sampled pairs must
equal the restatement.  Also recorded: the share of pairs with lb == ub (the distance is then
exact) and the histogram of ub - lb.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def _stores():
    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.data import synthetic_graph
    from graphembedding_amd.ged import store_of_graphs
    a = load_graph_set('syn_aids700nef').store
    rng = np.random.default_rng(32)
    gs = [synthetic_graph(rng, int(rng.integers(5, 31)), gid) for gid in range(2048)]
    return (('aids700nef', a), ('cap32', store_of_graphs(gs, n_max=32)))


class Grid(object):
    """One all-pairs grid with its buffers; run() is the bare C-ABI call."""

    def __init__(self, store, device, bounds=True, both=True):
        import torch
        from graphembedding_amd import _lib
        self._lib = _lib
        self.store, self.both = store, both
        self.dev = store.to_device(device)
        self.G = G = len(store)
        nbytes = _lib.ged_grid_workspace_bytes(G, G, store.n_max)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        self.ub = torch.empty((G, G), dtype=torch.int32, device=device)
        self.lb = torch.empty((G, G), dtype=torch.int32, device=device) if bounds else None
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self):
        self._lib.ged_grid(self.dev, self.store.n_max, None, self.G, None, self.G, self.both,
                           self.ub, self.G, self.lb, None, self.status, self.ws)

    def timed(self):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


def _stats(ms, pairs):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return dict(ms_median=med, ms_min=ms[0], ms_max=ms[-1], repeats=len(ms),
                pairs_per_s=pairs / (med * 1e-3))


def _host(store, sample, ub, lb):
    """Host pairs/s on the sampled pairs, after checking the device against the restatement."""
    import _ged_restatement as R
    from scipy.optimize import linear_sum_assignment
    ref = R.GridReference(store)
    t = time.perf_counter()
    for a, b in sample:
        u = min(ref.pair(a, b)[0], ref.pair(b, a)[0])
        assert (u, ref.pair(a, b)[1]) == (int(ub[a, b]), int(lb[a, b])), (a, b)
    rest_s = time.perf_counter() - t
    graphs = [ref.graph(g) for g in range(len(store))]
    t = time.perf_counter()
    for a, b in sample:
        g1, g2 = graphs[a], graphs[b]
        n1, n2 = len(g1[0]), len(g2[0])
        for x, y, nx_, ny in ((g1, g2, n1, n2), (g2, g1, n2, n1)):
            r, c = linear_sum_assignment(R.cost_matrix(x, y, 1))
            p = np.empty(nx_ + ny, dtype=np.int64)
            p[c] = r
            R.induced_cost(x, y, R.phi_of(p, nx_, ny))
        C2 = R.cost_matrix(g1, g2, 2)
        r, c = linear_sum_assignment(C2)
        assert (int(C2[r, c].sum()) + 1) // 2 == int(lb[a, b])
    scipy_s = time.perf_counter() - t
    return dict(sample=len(sample), scipy_pairs_per_s=len(sample) / scipy_s,
                restatement_pairs_per_s=len(sample) / rest_s)


def main():
    import torch
    from graphembedding_amd.build import build_hip
    build_hip()
    device = torch.device('cuda:0')
    repeats, n_sample = _arg('--repeats', 7), _arg('--sample', 300)
    stores = _stores()
    full = [Grid(s, device) for _, s in stores]
    part = [Grid(s, device, bounds=False, both=False) for _, s in stores]
    for g in full + part:   # warm-up
        g.run()
    torch.cuda.synchronize()
    t_full, t_part = [[] for _ in full], [[] for _ in part]
    for _ in range(repeats):
        for k in range(len(full)):
            t_full[k].append(full[k].timed())
        for k in range(len(part)):
            t_part[k].append(part[k].timed())
    grids = []
    for k, (name, store) in enumerate(stores):
        g = full[k]
        assert int(g.status.item()) == 0
        ub, lb = g.ub.cpu().numpy(), g.lb.cpu().numpy()
        G = g.G
        assert np.array_equal(ub, ub.T) and not np.diag(ub).any() and (lb <= ub).all()
        rng = np.random.default_rng(k)
        sample = [(int(a), int(b)) for a, b in rng.integers(0, G, size=(n_sample, 2))]
        gap = (ub - lb).astype(np.int64)
        out = dict(grid=name, graphs=G, pairs=G * G, n_max=store.n_max,
                   nodes_min=int(store.n.min()), nodes_max=int(store.n.max()),
                   both_orders_and_lb=_stats(t_full[k], G * G),
                   ub_only_one_order=_stats(t_part[k], G * G),
                   host=_host(store, sample, ub, lb),
                   exact_share=float((gap == 0).mean()),
                   gap_histogram=np.bincount(gap.reshape(-1)).tolist(),
                   ub_mean=float(ub.mean()), lb_mean=float(lb.mean()))
        h = out['host']
        dev = out['both_orders_and_lb']['pairs_per_s']
        h['scipy_grid_seconds_extrapolated'] = G * G / h['scipy_pairs_per_s']
        h['device_over_scipy'] = dev / h['scipy_pairs_per_s']
        h['device_over_restatement'] = dev / h['restatement_pairs_per_s']
        grids.append(out)
    result = dict(bench='ged_grid', gpu=torch.cuda.get_device_name(0),
                  packing='one pair per wavefront (sub-wave packing not tried)', grids=grids)
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
