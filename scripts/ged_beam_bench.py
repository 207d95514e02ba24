"""The beam-search GED (include/siamese_ged_beam.h) on a C4-like grid (GPU only).

    python scripts/ged_beam_bench.py [--repeats 5] [--graphs 512] [--sample 12] [--out FILE.json]

One grid: the first --graphs graphs of syn_aids10knef (seed 123: 5 .. 30 nodes, 29 types) in a
capacity-32 store, all ordered pairs, one sg_ged_beam_grid call (two launches) per width in
(1, 10, 80), with lb_out and expanded_out and no map.  The yardstick is sg_ged_grid on the same
grid (both orders and the lower bound: the seed alone).  Device times are HIP events around the
call with every buffer allocated beforehand, after one warm-up call of each; the repeats
alternate between the calls so a drift of the clocks falls on all; median with min .. max.

Recorded besides the times: the mean ub of each call, the share of pairs proven (lb == ub), the
share where ub fell below the bipartite ub, and the states expanded.  Before timing, --sample
random searched pairs must equal the restatement (tests/_ged_beam_restatement.py) in ub, lb and
expanded at width 10.  Nothing is gated on a ratio.  Prints one JSON line.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WIDTHS = (1, 10, 80)


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


class Grid(object):
    """The all-pairs grid with its buffers; run() is the bare C-ABI call (width None: the
    bipartite call)."""

    def __init__(self, store, device, width):
        import torch
        from graphembedding_amd import _lib
        self._lib, self.store, self.width = _lib, store, width
        self.dev = store.to_device(device)
        self.G = G = len(store)
        nbytes = _lib.ged_beam_grid_workspace_bytes(G, G, store.n_max)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        self.ub = torch.empty((G, G), dtype=torch.int32, device=device)
        self.lb = torch.empty((G, G), dtype=torch.int32, device=device)
        self.ex = torch.empty((G, G), dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self):
        if self.width is None:
            self._lib.ged_grid(self.dev, self.store.n_max, None, self.G, None, self.G, True,
                               self.ub, self.G, self.lb, None, self.status, self.ws)
        else:
            self._lib.ged_beam_grid(self.dev, self.store.n_max, None, self.G, None, self.G,
                                    self.width, self.ub, self.G, self.lb, None, self.ex,
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


def c4_like_graphs(count, seed=123):
    """The first `count` graphs of data.synthetic_graphs('syn_aids10knef', seed)."""
    from graphembedding_amd.data import SYNTHETIC, synthetic_graph
    _, _, lo, hi, nt = SYNTHETIC['syn_aids10knef']
    rng = np.random.default_rng(seed)
    return [synthetic_graph(rng, int(rng.integers(lo, hi + 1)), gid, nt, p_extra=0.15)
            for gid in range(count)]


def main():
    import torch
    from graphembedding_amd.build import build_hip
    from graphembedding_amd.ged import store_of_graphs
    build_hip()
    device = torch.device('cuda:0')
    repeats, n_sample, count = _arg('--repeats', 5), _arg('--sample', 12), _arg('--graphs', 512)
    store = store_of_graphs(c4_like_graphs(count), n_max=32)
    grids = {w: Grid(store, device, w) for w in WIDTHS + (None,)}
    for g in grids.values():   # warm-up
        g.run()
    torch.cuda.synchronize()
    times = {w: [] for w in grids}
    for _ in range(repeats):
        for w, g in grids.items():
            times[w].append(g.timed())
    G = len(store)
    n = np.asarray(store.n)
    ub0, lb0 = grids[None].ub.cpu().numpy(), grids[None].lb.cpu().numpy()
    assert int(grids[None].status.item()) == 0
    result = dict(
        bench='ged_beam_grid', gpu=torch.cuda.get_device_name(0), grid='aids10knef-like',
        graphs=G, pairs=G * G, n_max=store.n_max, nodes_min=int(n.min()), nodes_max=int(n.max()),
        nodes_mean=float(n.mean()), packing='one pair per wavefront, one lane per child',
        bipartite_both_orders_and_lb=dict(_stats(times[None], G * G), ub_mean=float(ub0.mean()),
                                          lb_mean=float(lb0.mean()),
                                          proven_share=float((ub0 == lb0).mean())))
    for w in WIDTHS:
        g = grids[w]
        assert int(g.status.item()) == 0
        ub, lb, ex = (t.cpu().numpy() for t in (g.ub, g.lb, g.ex))
        assert (lb <= ub).all() and (ub <= ub0).all() and ((lb == ub) | (lb == lb0)).all()
        assert (ex <= 1 + (n[:, None] - 1) * w).all()
        if w == 10:   # the sampled searched pairs against the restatement
            import _ged_beam_restatement as B
            ref = B.BeamGridReference(store)
            rng = np.random.default_rng(0)
            cand = np.argwhere(ex > 0)
            sample = cand[rng.permutation(len(cand))[:n_sample]]
            for a, b in sample:
                want = ref.pair(int(a), int(b), w)
                assert (want[0], want[1], want[3]) == (int(ub[a, b]), int(lb[a, b]),
                                                       int(ex[a, b])), (a, b)
            result['checked_against_restatement'] = int(len(sample))
        result['width_{}'.format(w)] = dict(
            _stats(times[w], G * G), ub_mean=float(ub.mean()),
            proven_share=float((ub == lb).mean()), proven_pairs=int((ub == lb).sum()),
            ub_below_bipartite_share=float((ub < ub0).mean()),
            searched_pairs=int((ex > 0).sum()), expanded_sum=int(ex.sum()),
            expanded_max=int(ex.max()),
            expanded_per_s=float(ex.sum() / (sorted(times[w])[len(times[w]) // 2] * 1e-3)))
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
