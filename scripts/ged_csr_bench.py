"""The bipartite GED bounds for graph-store (CSR) graphs (include/siamese_ged_csr.h) at three
graph sizes (GPU only).

    python scripts/ged_csr_bench.py [--graphs 64] [--repeats 3] [--rounds 2] [--scipy 64]
                                    [--out FILE.json]

Three seeded sets of --graphs synthetic graphs (data.synthetic_graph, 29 types, a spanning tree
plus 1.5 extra edges per node on average): n in 48 .. 80 (about 64), 256 .. 320 (about 288, the
C5 mean) and 480 .. 512.  Per set:

  grid     one sg_csr_ged_grid call over all ordered pairs, both orders, lb_out, no map: HIP
           events around the call with every buffer allocated beforehand, after one warm-up
           call; median (min .. max) of --repeats; pairs/s.
  rounds   --rounds pairs of the set solved by the numpy restatement
           (tests/_ged_csr_restatement.py), which counts its solver rounds over the three solves
           of a pair (1->2 and 2->1 at w = 1, 1->2 at w = 2) and must equal the device's ub and
           lb; the same pair as a 1 x 1 grid on the device, alone on the card: ns per round of
           one wavefront = the call's time over those rounds.  This is the figure that sizes a
           time limit: a pair's time is its rounds times it, however many pairs run beside it.
           The known ceiling is 3 solves of at most N^2 rounds each.
  scipy    the only baseline available: scipy.optimize.linear_sum_assignment on the same three
           matrices of --scipy sampled pairs, 16 host processes (before the GPU is opened),
           matrices built beforehand; pairs/s.  It solves the assignment problems only: no
           induced cost.

Nothing is gated on a ratio.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SETS = (('n64', 48, 80), ('n288', 256, 320), ('n512', 480, 512))
HOST_PROCS = 16


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def graphs_of(lo, hi, count, seed):
    from graphembedding_amd.data import synthetic_graph
    rng = np.random.default_rng(seed)
    out = []
    for gid in range(count):
        n = int(rng.integers(lo, hi + 1))
        out.append(synthetic_graph(rng, n, gid, 29, p_extra=1.5 / max(n - 1, 1)))
    return out


def _scipy_pair(mats):
    from scipy.optimize import linear_sum_assignment
    t0 = time.perf_counter()
    opts = []
    for M in mats:
        r, c = linear_sum_assignment(M)
        opts.append(int(M[r, c].sum()))
    return time.perf_counter() - t0, opts


def scipy_baseline(ref, pairs):
    """Wall time of the three assignment problems of every sampled pair over 16 processes."""
    import multiprocessing as mp

    import _ged_csr_restatement as C
    work = []
    for a, b in pairs:
        ga, gb = ref.graph(a), ref.graph(b)
        work.append([C.cost_matrix(ga, gb, 1), C.cost_matrix(gb, ga, 1), C.cost_matrix(ga, gb, 2)])
    with mp.get_context('fork').Pool(HOST_PROCS) as pool:
        pool.map(_scipy_pair, work[:HOST_PROCS])     # the workers are up
        t0 = time.perf_counter()
        res = pool.map(_scipy_pair, work, chunksize=1)
        wall = time.perf_counter() - t0
    return dict(pairs=len(pairs), processes=HOST_PROCS, wall_s=wall, pairs_per_s=len(pairs) / wall,
                solve_s_mean=float(np.mean([r[0] for r in res]) / 3)), [r[1] for r in res]


class Grid(object):
    """A q x db grid of a CsrStore with its buffers; run() is the bare C-ABI call."""

    def __init__(self, store, device, q=None, db=None):
        import torch
        from graphembedding_amd import _lib
        self._lib, self.store = _lib, store
        self.struct = store.to_device(device)
        self.q = None if q is None else torch.as_tensor(q, dtype=torch.int32, device=device)
        self.db = None if db is None else torch.as_tensor(db, dtype=torch.int32, device=device)
        self.m = len(store) if q is None else len(q)
        self.n = len(store) if db is None else len(db)
        nbytes = _lib.csr_ged_grid_workspace_bytes(self.m, self.n, store.n_max)
        self.ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=device)
        self.ub = torch.empty((self.m, self.n), dtype=torch.int32, device=device)
        self.lb = torch.empty((self.m, self.n), dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self):
        self._lib.csr_ged_grid(self.struct, self.q, self.m, self.db, self.n, True, self.ub,
                               self.n, self.lb, None, self.status, self.ws)

    def timed(self):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


def _stats(ms):
    ms = sorted(ms)
    return dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], repeats=len(ms))


def count_rounds(ref, a, b):
    """(rounds of the three solves, ub over both orders, lb) of the restatement."""
    import _ged_csr_restatement as C
    ga, gb = ref.graph(a), ref.graph(b)
    rounds, cnt = 0, [0]
    p, _ = C.lsap(C.cost_matrix(ga, gb, 1), cnt)
    rounds += cnt[0]
    ub = C.induced_cost(ga, gb, C.phi_of(p, len(ga[0]), len(gb[0])))
    p, _ = C.lsap(C.cost_matrix(gb, ga, 1), cnt)
    rounds += cnt[0]
    ub = min(ub, C.induced_cost(gb, ga, C.phi_of(p, len(gb[0]), len(ga[0]))))
    _, opt = C.lsap(C.cost_matrix(ga, gb, 2), cnt)
    rounds += cnt[0]
    return rounds, ub, (opt + 1) // 2


def main():
    import _ged_csr_restatement as C
    from graphembedding_amd.build import build_hip
    from graphembedding_amd.ged import csr_store_of_graphs
    build_hip()
    count, repeats = _arg('--graphs', 64), _arg('--repeats', 3)
    n_rounds, n_scipy = _arg('--rounds', 2), _arg('--scipy', 64)
    sets, host = {}, {}
    for k, (name, lo, hi) in enumerate(SETS):       # the host side first: no GPU is open yet
        store = csr_store_of_graphs(graphs_of(lo, hi, count, 500 + k))
        ref = C.GridReference(store)
        rng = np.random.default_rng(k)
        pairs = [(int(a), int(a + 1 + d) % count)     # a != b
                 for a, d in rng.integers(0, count - 1, size=(n_scipy, 2))]
        base, opts = scipy_baseline(ref, pairs)
        counted = [pairs[i] + count_rounds(ref, *pairs[i]) for i in range(n_rounds)]
        sets[name] = (store, pairs, opts, counted)
        host[name] = base
    import torch
    device = torch.device('cuda:0')
    result = dict(bench='csr_ged_grid', gpu=torch.cuda.get_device_name(0), graphs=count,
                  pairs=count * count, both_orders=1, lb=1,
                  ceiling='3 solves of at most N^2 rounds per pair')
    for name, (store, pairs, opts, counted) in sets.items():
        n = np.asarray(store.n)
        grid = Grid(store, device)
        grid.run()
        torch.cuda.synchronize()
        ms = [grid.timed() for _ in range(repeats)]
        assert int(grid.status.item()) == 0
        ub, lb = grid.ub.cpu().numpy(), grid.lb.cpu().numpy()
        assert (lb <= ub).all() and np.array_equal(ub, ub.T) and not np.diag(ub).any()
        for (a, b), o in zip(pairs, opts):          # scipy's optimum of the w = 2 matrix
            assert lb[a, b] == (o[2] + 1) // 2, (name, a, b)
        per_round = []
        for a, b, rounds, wub, wlb in counted:
            assert (int(ub[a, b]), int(lb[a, b])) == (wub, wlb), (name, a, b)
            one = Grid(store, device, [a], [b])
            one.run()
            torch.cuda.synchronize()
            t = _stats([one.timed() for _ in range(repeats)])['ms_median']
            N = int(n[a] + n[b])
            per_round.append(dict(n1=int(n[a]), n2=int(n[b]), rounds=rounds,
                                  rounds_ceiling=3 * N * N, ms=t, ns_per_round=t * 1e6 / rounds))
        st = _stats(ms)
        result[name] = dict(
            st, n_max=store.n_max, nodes_min=int(n.min()), nodes_max=int(n.max()),
            nodes_mean=float(n.mean()), pairs_per_s=count * count / (st['ms_median'] * 1e-3),
            ub_mean=float(ub.mean()), lb_mean=float(lb.mean()), one_wavefront=per_round,
            scipy_16_processes=host[name])
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
