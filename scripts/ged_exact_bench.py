"""The budgeted exact GED (include/siamese_ged_exact.h) on the AIDS700nef-shaped grid (GPU only).

    python scripts/ged_exact_bench.py [--repeats 5] [--budget 1048576] [--sample 40] [--out FILE.json]

One grid: syn_aids700nef, 700 x 700 = 490,000 pairs of 5 .. 10 nodes, capacity 10, one
sg_ged_exact_grid call (two launches) at the default budget of 2^20 expansions per pair, with
lb_out and expansions_out and no map.  For scale the same grid through sg_ged_grid (both
orders and the lower bound: the seed alone).  Device times are HIP events around the call with
every buffer allocated beforehand, after one warm-up call of each; the repeats alternate
between the two calls so a drift of the clocks falls on both; median with min .. max.

Recorded besides the times: the share of pairs proven (lb == ub), the share the bipartite
bounds had already closed, the pairs left unproven with their node counts, the histogram of
expansions per pair by powers of two, the largest count and the sum, and how far ub fell below
the bipartite ub.  Before timing, --sample random searched pairs must equal the restatement
(tests/_ged_exact_restatement.py) in ub, lb and expansions.  Prints one JSON line.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


class Grid(object):
    """The all-pairs grid with its buffers; run() is the bare C-ABI call (budget None: the
    bipartite call)."""

    def __init__(self, store, device, budget):
        import torch
        from graphembedding_amd import _lib
        self._lib, self.store, self.budget = _lib, store, budget
        self.dev = store.to_device(device)
        self.G = G = len(store)
        nbytes = _lib.ged_exact_grid_workspace_bytes(G, G, store.n_max)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        self.ub = torch.empty((G, G), dtype=torch.int32, device=device)
        self.lb = torch.empty((G, G), dtype=torch.int32, device=device)
        self.ex = torch.empty((G, G), dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self):
        if self.budget is None:
            self._lib.ged_grid(self.dev, self.store.n_max, None, self.G, None, self.G, True,
                               self.ub, self.G, self.lb, None, self.status, self.ws)
        else:
            self._lib.ged_exact_grid(self.dev, self.store.n_max, None, self.G, None, self.G,
                                     self.budget, self.ub, self.G, self.lb, None, self.ex,
                                     self.status, self.ws)

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


def main():
    import torch
    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.build import build_hip
    from graphembedding_amd.ged import GED_EXACT_DEFAULT_BUDGET
    build_hip()
    device = torch.device('cuda:0')
    repeats, n_sample = _arg('--repeats', 5), _arg('--sample', 40)
    budget = _arg('--budget', GED_EXACT_DEFAULT_BUDGET)
    store = load_graph_set('syn_aids700nef').store
    exact, seed = Grid(store, device, budget), Grid(store, device, None)
    exact.run()   # warm-up
    seed.run()
    torch.cuda.synchronize()
    t_exact, t_seed = [], []
    for _ in range(repeats):
        t_exact.append(exact.timed())
        t_seed.append(seed.timed())
    assert int(exact.status.item()) == 0 and int(seed.status.item()) == 0
    ub, lb, ex = (t.cpu().numpy() for t in (exact.ub, exact.lb, exact.ex))
    ub0, lb0 = seed.ub.cpu().numpy(), seed.lb.cpu().numpy()
    G = exact.G
    n = np.asarray(store.n)
    assert (lb <= ub).all() and (ub <= ub0).all() and (lb >= lb0).all() and (ex <= budget).all()
    proven = ub == lb
    # the sampled searched pairs against the restatement (cheap ones: the host is slow)
    import _ged_exact_restatement as X
    ref = X.ExactGridReference(store)
    rng = np.random.default_rng(0)
    cand = np.argwhere((ex > 0) & (ex <= 5000))
    sample = cand[rng.permutation(len(cand))[:n_sample]]
    for a, b in sample:
        want = ref.pair(int(a), int(b), budget)
        assert (want[0], want[1], want[3]) == (int(ub[a, b]), int(lb[a, b]), int(ex[a, b])), (a, b)
    unproven = np.argwhere(~proven)
    sizes = {}
    for a, b in unproven:
        k = '{}x{}'.format(int(n[a]), int(n[b]))
        sizes[k] = sizes.get(k, 0) + 1
    bins = np.zeros(26, dtype=np.int64)   # bin 0: no search; bin i: 2^(i-1) <= expansions < 2^i
    np.add.at(bins, np.where(ex > 0, np.floor(np.log2(np.maximum(ex, 1))).astype(np.int64) + 1, 0), 1)
    result = dict(
        bench='ged_exact_grid', gpu=torch.cuda.get_device_name(0), grid='aids700nef', graphs=G,
        pairs=G * G, n_max=store.n_max, nodes_min=int(n.min()), nodes_max=int(n.max()),
        budget=budget, packing='one pair per wavefront, one lane per child',
        exact=_stats(t_exact, G * G), bipartite_both_orders_and_lb=_stats(t_seed, G * G),
        proven_share=float(proven.mean()), proven_pairs=int(proven.sum()),
        closed_by_the_bipartite_bounds_share=float((ub0 == lb0).mean()),
        unproven_pairs=int((~proven).sum()), unproven_by_node_counts=sizes,
        searched_pairs=int((ex > 0).sum()),
        expansions_histogram_pow2=bins.tolist(), expansions_max=int(ex.max()),
        expansions_sum=int(ex.sum()), expansions_mean_of_searched=float(ex[ex > 0].mean()),
        expansions_per_s=float(ex.sum() / (sorted(t_exact)[len(t_exact) // 2] * 1e-3)),
        ub_below_bipartite_share=float((ub < ub0).mean()),
        ub_mean=float(ub.mean()), bipartite_ub_mean=float(ub0.mean()),
        bipartite_lb_mean=float(lb0.mean()), checked_against_restatement=int(len(sample)))
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
