"""Embed-once training against the pairwise step on the AIDS700nef-shaped set (GPU only).

    python scripts/grid_train_bench.py [--repeats 5] [--iters 20] [--out FILE.json]
    python scripts/grid_train_bench.py --dropout [--repeats 5] [--iters 20] [--out FILE.json]

One full all-pairs training step (forward, backward, Adam) of syn_aids700nef at dropout 0,
timed `--repeats` times alternated in one process (device events, warmed up):
  (a) AllPairsGrid.train_step: embed 700 graphs, the 700 x 700 NTN grid forward + backward,
      one node-stack backward per graph, Adam; and its parts alone (embed, grid fwd+bwd,
      the role sum, embed backward, Adam);
  (b) the yardstick, the path the tree had for this objective before: the class-ordered
      fused sg_train_step over the 490,000 packed records at dropout 0;
  (c) sg_score_grid_fwd_bwd 4096 x 4096 on synthetic embeddings, next to sg_score_grid's
      forward of the same grid.
(a) and (b) compute the same loss and gradient (checked before timing: loss within 1e-4,
every variable's gradient within 1e-4 of its largest component).  The condition on (a) is
median(a) < median(b) - spread, spread = the larger max - min of the two over the repeats;
the ratio is reported, not asserted.  Prints one JSON line.

--dropout measures what graph-keyed dropout (include/siamese_embed_drop.h) costs instead:
the same step alternated between (d0) AllPairsGrid at dropout 0, as above, (dg) AllPairsGrid
with dropout='graph' at dropout 0.1 and (dp) the pairwise fused step over the 490,000
records at dropout 0.1, with the embed forward and backward of (d0) and (dg) alone.  The
three compute different objectives (no masks, one mask set per graph, one per pair); only
their times are compared.  No threshold: the medians and spreads are reported.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def timed(fn, iters):
    """msec per call of fn over `iters` back-to-back calls (device events)."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def dropout_main():
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.allpairs import AllPairsGrid, AllPairsShard, load_graph_set
    from graphembedding_amd.config import Flags
    from graphembedding_amd.model_mse import SiameseGCNTNMSE
    if not torch.cuda.is_available():
        raise SystemExit('grid_train_bench needs a GPU (there is no CPU fallback)')
    dev = torch.device('cuda', 0)
    repeats, iters = _arg('--repeats', 5), _arg('--iters', 20)
    f0, f1 = Flags(dropout=0.0), Flags(dropout=0.1)
    gs = load_graph_set('syn_aids700nef', n_max=10)
    G = len(gs.mgs)
    labels = gs.label_matrix(f0.yeta)
    m0 = SiameseGCNTNMSE(gs.d_in, f0, device=dev, n_max=gs.n_max)
    mg = SiameseGCNTNMSE(gs.d_in, f1, device=dev, n_max=gs.n_max, params=m0.flat_params())
    mp = SiameseGCNTNMSE(gs.d_in, f1, device=dev, n_max=gs.n_max, params=m0.flat_params())
    grid0, gridg = AllPairsGrid(gs, labels, dev), AllPairsGrid(gs, labels, dev, dropout='graph')
    gp0, gpg = grid0.problem(m0), gridg.problem(mg)
    batch = AllPairsShard(gs, labels, device=dev).batch(mp)   # class-ordered (balance)
    assert mp.kernel_path == 1 and batch.cls is not None and mg.sg.keep_prob < 1.0
    U, nmax = int(gp0.uniq.numel()), m0.n_max

    def d0_embed():
        _lib.embed(m0.sg, gp0.store_dev, nmax, gp0.uniq, U, m0.params, gp0.emb, gp0.status)

    def dg_embed():
        _lib.embed_drop(mg.sg, gpg.store_dev, nmax, gpg.uniq, U, 0, mg.params, 1, gpg.emb,
                        gpg.status)

    def d0_embed_bwd():
        _lib.embed_bwd(m0.sg, gp0.store_dev, nmax, gp0.uniq, U, m0.params, gp0.g_emb, m0.grad,
                       gp0.ws_embed, gp0.status)

    def dg_embed_bwd():
        _lib.embed_drop_bwd(mg.sg, gpg.store_dev, nmax, gpg.uniq, U, 0, mg.params, 1, gpg.g_emb,
                            mg.grad, gpg.ws_embed, gpg.status)

    cases = [('grid_step_d0', lambda: grid0.train_step(m0, sync=False)),
             ('grid_step_graph_d01', lambda: gridg.train_step(mg, sync=False)),
             ('pairwise_step_d01', lambda: mp.train_step(batch, sync=False)),
             ('embed_d0', d0_embed), ('embed_drop_d01', dg_embed),
             ('embed_bwd_d0', d0_embed_bwd), ('embed_drop_bwd_d01', dg_embed_bwd)]
    for _, fn in cases:          # warm-up of every shape
        timed(fn, 3)
    ms = {k: [] for k, _ in cases}
    for _ in range(repeats):     # alternated
        for k, fn in cases:
            ms[k].append(timed(fn, iters))
    torch.cuda.synchronize()
    gp0.check()
    gpg.check()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(graphs=G, pairs=G * G, repeats=repeats, iters=iters, msec=ms, msec_median=med,
               spread_msec={k: max(v) - min(v) for k, v in ms.items()},
               graph_dropout_over_dropout0=med['grid_step_graph_d01'] / med['grid_step_d0'],
               pairwise_over_graph_dropout=med['pairwise_step_d01'] / med['grid_step_graph_d01'],
               device=torch.cuda.get_device_name(0), one_box=True)
    line = json.dumps(res)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


def main():
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.allpairs import AllPairsGrid, AllPairsShard, load_graph_set
    from graphembedding_amd.config import Flags
    from graphembedding_amd.model_mse import SiameseGCNTNMSE, param_shapes
    if not torch.cuda.is_available():
        raise SystemExit('grid_train_bench needs a GPU (there is no CPU fallback)')
    dev = torch.device('cuda', 0)
    repeats, iters = _arg('--repeats', 5), _arg('--iters', 20)
    flags = Flags(dropout=0.0)
    gs = load_graph_set('syn_aids700nef', n_max=10)
    G = len(gs.mgs)
    labels = gs.label_matrix(flags.yeta)
    mg = SiameseGCNTNMSE(gs.d_in, flags, device=dev, n_max=gs.n_max)
    mp = SiameseGCNTNMSE(gs.d_in, flags, device=dev, n_max=gs.n_max, params=mg.flat_params())
    grid = AllPairsGrid(gs, labels, dev)
    gp = grid.problem(mg)
    shard = AllPairsShard(gs, labels, device=dev)
    batch = shard.batch(mp)            # class-ordered (balance)
    assert mp.kernel_path == 1 and batch.cls is not None

    # same objective: loss and per-variable gradient of (a) against (b)
    grid.fwd_bwd(mg)
    mp.fwd_bwd(batch, seed=1)
    torch.cuda.synchronize()
    gp.check()
    la, lb = float(mg.loss_buf[0].item()), float(mp.loss_buf[0].item())
    assert abs(la - lb) <= 1e-4 * max(1.0, abs(lb)), (la, lb)
    ga, gb = mg.grad.cpu().numpy().astype(np.float64), mp.grad.cpu().numpy().astype(np.float64)
    off, rel = 0, {}
    for li, name, shape in param_shapes(mg.layers, gs.d_in):
        k = int(np.prod(shape))
        scale = max(float(np.abs(gb[off:off + k]).max()), 1e-30)
        rel['{}.{}'.format(li, name)] = float(np.abs(ga[off:off + k] - gb[off:off + k]).max()) / scale
        off += k
    assert max(rel.values()) <= 1e-4, rel

    U, nmax = int(gp.uniq.numel()), mg.n_max

    def a_step():
        grid.train_step(mg, sync=False)

    def b_step():
        mp.fwd_bwd_adam(batch, seed=1)

    def a_embed():
        _lib.embed(mg.sg, gp.store_dev, nmax, gp.uniq, U, mg.params, gp.emb, gp.status)

    def a_grid():
        _lib.score_grid_fwd_bwd(mg.sg, gp.emb, gp.emb, G, G, mg.params, gp.labels, G, G * G,
                                gp.y_stats, True, None, G, gp.g_q, gp.g_db, mg.grad,
                                mg.loss_buf, gp.ws_grid)

    def a_sum():
        torch.add(gp.g_q, gp.g_db, out=gp.g_emb)

    def a_embed_bwd():
        _lib.embed_bwd(mg.sg, gp.store_dev, nmax, gp.uniq, U, mg.params, gp.g_emb, mg.grad,
                       gp.ws_embed, gp.status)

    def a_adam():
        mg.apply_adam()

    # (c) 4096 x 4096 from synthetic embeddings: the adjoint next to the forward grid
    N, E = 4096, mg.embed_dim
    rng = np.random.default_rng(0)
    syn = torch.from_numpy(rng.uniform(0, 1, size=(N, E)).astype(np.float32)).to(dev)
    lab_c = torch.from_numpy(rng.uniform(0, 1, size=(N, N)).astype(np.float32)).to(dev)
    ws_f = torch.empty(_lib.score_grid_workspace_bytes(mg.sg, N) // 4 + 1, dtype=torch.float32,
                       device=dev)
    bwd_bytes = _lib.score_grid_bwd_workspace_bytes(mg.sg, N, N)
    ws_b = torch.empty(bwd_bytes // 4 + 1, dtype=torch.float32, device=dev)
    out_c = torch.empty((N, N), dtype=torch.float32, device=dev)
    gq_c, gdb_c = torch.empty_like(syn), torch.empty_like(syn)
    grad_c, loss_c = torch.empty_like(mg.grad), torch.empty(1, dtype=torch.float32, device=dev)

    def c_fwd():
        _lib.score_grid(mg.sg, syn, syn, N, N, mg.params, True, out_c, N, ws_f)

    def c_fwd_bwd():
        _lib.score_grid_fwd_bwd(mg.sg, syn, syn, N, N, mg.params, lab_c, N, N * N, gp.y_stats,
                                True, None, N, gq_c, gdb_c, grad_c, loss_c, ws_b)

    cases = [('grid_step_700', a_step), ('pairwise_step_700', b_step), ('embed_700', a_embed),
             ('grid_fwd_bwd_700', a_grid), ('role_sum_700', a_sum),
             ('embed_bwd_700', a_embed_bwd), ('adam', a_adam), ('grid_fwd_4096', c_fwd),
             ('grid_fwd_bwd_4096', c_fwd_bwd)]
    for _, fn in cases:          # warm-up of every shape
        timed(fn, 3)
    ms = {k: [] for k, _ in cases}
    for _ in range(repeats):     # alternated
        for k, fn in cases:
            ms[k].append(timed(fn, iters))
    torch.cuda.synchronize()
    gp.check()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = max(max(ms[k]) - min(ms[k]) for k in ('grid_step_700', 'pairwise_step_700'))
    parts = ('embed_700', 'grid_fwd_bwd_700', 'role_sum_700', 'embed_bwd_700', 'adam')
    res = dict(graphs=G, pairs=G * G, embed_dim=E, repeats=repeats, iters=iters,
               loss_grid=la, loss_pairwise=lb, max_rel_grad_diff=max(rel.values()),
               msec=ms, msec_median=med, spread_msec=spread,
               grid_faster_beyond_spread=bool(med['grid_step_700'] <
                                              med['pairwise_step_700'] - spread),
               pairwise_over_grid=med['pairwise_step_700'] / med['grid_step_700'],
               share_of_parts={k: med[k] / sum(med[p] for p in parts) for k in parts},
               grid_4096_bwd_workspace_MB=bwd_bytes / 1e6,
               grid_4096_fwd_bwd_over_fwd=med['grid_fwd_bwd_4096'] / med['grid_fwd_4096'],
               device=torch.cuda.get_device_name(0), one_box=True)
    line = json.dumps(res)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    dropout_main() if '--dropout' in sys.argv[1:] else main()
