"""The GED refinement (include/siamese_ged_refine.h) next to the bipartite bounds and the beam
search on the same grids (GPU only).

    python scripts/ged_refine_bench.py [--repeats 5] [--graphs 512] [--sample 12] [--out FILE.json]

Two grids, all ordered pairs of each: syn_aids700nef (seed 123: 700 graphs of at most 10 nodes, a
capacity-10 store) and the first --graphs graphs of syn_aids10knef (5 .. 30 nodes, 29 types) in a
capacity-32 store.  Three calls per grid, each with lb_out and its counter and no map:
sg_ged_grid (both orders and the lower bound: the seed alone), sg_ged_beam_grid at width 80 and
sg_ged_refine_grid at ged.GED_REFINE_DEFAULT_MOVES.  Device times are HIP events around a window
of calls (as many as fill about 0.2 s, found from one timed call after the warm-up) with every
buffer allocated beforehand; the repeats alternate between the three calls so a drift of the
clocks falls on all; median with min .. max, per call.

Recorded besides the times: pairs/s, the slack sum(ub - lb), the pairs proven (lb == ub), the
pairs where ub fell below the bipartite ub, and the largest counter (states expanded, moves
accepted).  Before timing, --sample random refined pairs of each grid must equal the restatement
(tests/_ged_refine_restatement.py) in ub, lb and moves.  Nothing is gated on a ratio.  Prints one
JSON line.
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

BEAM_WIDTH = 80
WINDOW_MS = 200.0
CALLS = ('bp', 'lbeam80', 'bpswap')


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


class Grid(object):
    """The all-pairs grid of a store with its buffers; run() is the bare C-ABI call."""

    def __init__(self, store, device, call, moves):
        import torch
        from graphembedding_amd import _lib
        self._lib, self.store, self.call, self.moves = _lib, store, call, moves
        self.dev = store.to_device(device)
        self.G = G = len(store)
        nbytes = _lib.ged_refine_grid_workspace_bytes(G, G, store.n_max)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        self.ub = torch.empty((G, G), dtype=torch.int32, device=device)
        self.lb = torch.empty((G, G), dtype=torch.int32, device=device)
        self.count = torch.zeros((G, G), dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.inner = 1

    def run(self):
        L, G, nm = self._lib, self.G, self.store.n_max
        if self.call == 'bp':
            L.ged_grid(self.dev, nm, None, G, None, G, True, self.ub, G, self.lb, None,
                       self.status, self.ws)
        elif self.call == 'lbeam80':
            L.ged_beam_grid(self.dev, nm, None, G, None, G, BEAM_WIDTH, self.ub, G, self.lb, None,
                            self.count, self.status, self.ws)
        else:
            L.ged_refine_grid(self.dev, nm, None, G, None, G, self.moves, self.ub, G, self.lb,
                              None, self.count, self.status, self.ws)

    def timed(self):
        """ms per call over a window of self.inner calls."""
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(self.inner):
            self.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / self.inner


def _stats(ms, pairs, inner):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return dict(ms_median=med, ms_min=ms[0], ms_max=ms[-1], repeats=len(ms),
                calls_per_window=inner, pairs_per_s=pairs / (med * 1e-3))


def measure(name, store, device, repeats, n_sample, moves):
    import torch

    import _ged_refine_restatement as F
    grids = {c: Grid(store, device, c, moves) for c in CALLS}
    for g in grids.values():   # warm-up, then the window
        g.run()
        torch.cuda.synchronize()
        g.inner = max(1, min(100, int(math.ceil(WINDOW_MS / max(g.timed(), 1e-3)))))
    G = len(store)
    out = {c: tuple(t.cpu().numpy() for t in (g.ub, g.lb, g.count)) for c, g in grids.items()}
    assert all(int(g.status.item()) == 0 for g in grids.values())
    ub0, lb0, _ = out['bp']
    ub, lb, mv = out['bpswap']
    assert (lb == lb0).all() and (lb <= ub).all() and (ub <= ub0).all()
    ref = F.RefineGridReference(store)
    rng = np.random.default_rng(0)
    cand = np.argwhere(mv > 0)
    sample = cand[rng.permutation(len(cand))[:n_sample]]
    for a, b in sample:
        want = ref.pair(int(a), int(b), moves)
        assert (want[0], want[1], want[3]) == (int(ub[a, b]), int(lb[a, b]), int(mv[a, b])), (a, b)
    times = {c: [] for c in CALLS}
    for _ in range(repeats):
        for c, g in grids.items():
            times[c].append(g.timed())
    n = np.asarray(store.n)
    res = dict(grid=name, graphs=G, pairs=G * G, n_max=store.n_max, nodes_min=int(n.min()),
               nodes_max=int(n.max()), nodes_mean=float(n.mean()),
               checked_against_restatement=int(len(sample)))
    for c in CALLS:
        u, l, k = out[c]
        assert (l <= u).all() and (u <= ub0).all()
        res[c] = dict(_stats(times[c], G * G, grids[c].inner), slack_sum=int((u - l).sum()),
                      ub_mean=float(u.mean()), proven_pairs=int((u == l).sum()),
                      ub_below_bipartite_pairs=int((u < ub0).sum()))
        if c != 'bp':
            res[c]['counter'] = 'expanded' if c == 'lbeam80' else 'moves'
            res[c]['counter_max'] = int(k.max())
            res[c]['counter_sum'] = int(k.sum())
    res['bpswap']['ub_below_lbeam80_pairs'] = int((ub < out['lbeam80'][0]).sum())
    res['bpswap']['ub_above_lbeam80_pairs'] = int((ub > out['lbeam80'][0]).sum())
    return res


def main():
    import torch
    from ged_beam_bench import c4_like_graphs
    from graphembedding_amd.build import build_hip
    from graphembedding_amd.data import synthetic_graphs
    from graphembedding_amd.ged import GED_REFINE_DEFAULT_MOVES, store_of_graphs
    build_hip()
    device = torch.device('cuda:0')
    repeats, n_sample, count = _arg('--repeats', 5), _arg('--sample', 12), _arg('--graphs', 512)
    tr, te = synthetic_graphs('syn_aids700nef', 123)
    stores = (('aids700nef-like', store_of_graphs(tr + te, n_max=10)),
              ('aids10knef-like', store_of_graphs(c4_like_graphs(count), n_max=32)))
    result = dict(bench='ged_refine_grid', gpu=torch.cuda.get_device_name(0),
                  max_moves=GED_REFINE_DEFAULT_MOVES, beam_width=BEAM_WIDTH,
                  packing='one pair per wavefront, one lane per move, 64 moves per round',
                  grids=[measure(name, s, device, repeats, n_sample, GED_REFINE_DEFAULT_MOVES)
                         for name, s in stores])
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
