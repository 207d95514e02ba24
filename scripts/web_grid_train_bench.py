"""Embed-once training against the pairwise step on a C5-shaped graph store (GPU only).

    python scripts/web_grid_train_bench.py [--graphs 256] [--repeats 3] [--iters 3] [--out FILE.json]

One training step (forward, backward, Adam) over every pair of a store of `--graphs`
synthetic graphs of 200 .. 512 nodes, D = 512, K = 16, dropout 0, timed `--repeats` times
alternated in one process (device events, warmed up):
  (a) web_grid_train_step: sg_web_embed of the G graphs, sg_web_score_grid_fwd_bwd G x G,
      the role sum, sg_web_embed_bwd, Adam; and its parts alone;
  (b) the yardstick, the path the tree had for this objective before: the pairwise
      train_step (sg_web_fwd_bwd + Adam) over the same G·G pairs in chunks of 8192.
(a) and (b) compute the same loss and gradient (checked before timing: loss within 1e-4,
every variable's gradient within 1e-4 of its largest component).  No ratio is asserted: the
medians, the spreads (max - min over the repeats) and the ratio are reported.  Prints one
JSON line.

    python scripts/web_grid_train_bench.py --dropout 0.1 [--graphs 256] [--repeats 3] [--out FILE.json]

With --dropout P > 0 the same block runs with flags.dropout = P and times
  (c) web_grid_train_step(dropout='graph'): sg_web_embed_drop, the grid on the keep-1 copy of
      the model, the role sum, sg_web_embed_drop_bwd, Adam (masks keyed per graph)
against two yardsticks in the same run, alternated:
  (1) the pairwise train_step with dropout on (masks per pair), the only way the tree had to
      train such a model;
  (2) web_grid_train_step of the same model at dropout 0.
(c) and (1) draw different masks (per graph against per pair), so no loss is compared; (c) is
checked finite and its device status clean.  Medians, max - min and both ratios are reported.
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


D, K = 512, 16


def _setup(G, dropout):
    """The block's store, labels, encoder and flags at a dropout rate."""
    from graphembedding_amd.config import Flags
    from graphembedding_amd.data import synthetic_graph
    from graphembedding_amd.graphs import ModelGraph, NodeFeatureOneHotEncoder
    from graphembedding_amd.web import CsrStore
    rng = np.random.default_rng(0)
    graphs = [synthetic_graph(rng, int(rng.integers(200, D + 1)), gid, 29, p_extra=0.012)
              for gid in range(G)]
    enc = NodeFeatureOneHotEncoder(graphs, 'type').pin_sorted()
    mgs = [ModelGraph(g, enc) for g in graphs]
    flags = Flags(dropout=dropout,
                  layer_3='Padding:max_in_dims={},padding_value=0'.format(D),
                  layer_4='NTN:input_dim={},feature_map_dim={},inneract=relu,dropout=True,'
                          'bias=True'.format(D, K))
    store = CsrStore(mgs, enc.input_dim(), D)
    labels = rng.uniform(0.05, 1.0, size=(G, G)).astype(np.float32)
    return enc, flags, store, labels


def _all_pairs(G, dev):
    import torch
    ids = np.arange(G)
    return torch.from_numpy(np.stack([np.repeat(ids, G), np.tile(ids, G)],
                                     axis=1).astype(np.int32)).to(dev)


def _emit(res):
    line = json.dumps(res)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


def main_dropout(dropout):
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.model_mse import SiameseGCNTNMSE
    if not torch.cuda.is_available():
        raise SystemExit('web_grid_train_bench needs a GPU (there is no CPU fallback)')
    dev = torch.device('cuda', 0)
    G, repeats, iters = _arg('--graphs', 256), _arg('--repeats', 3), _arg('--iters', 3)
    enc, flags, store, labels = _setup(G, dropout)
    d_in = enc.input_dim()
    mg = SiameseGCNTNMSE(d_in, flags, device=dev, n_max=D)
    prm = mg.flat_params()
    mp = SiameseGCNTNMSE(d_in, flags, device=dev, n_max=D, params=prm)
    m0 = SiameseGCNTNMSE(d_in, flags.copy(dropout=0.0), device=dev, n_max=D, params=prm)
    assert mg.is_web and mg.sg.keep_prob < 1.0 and m0.sg.keep_prob == 1.0
    gp = mg.web_grid_problem(store, labels, dropout='graph')
    gp0 = m0.web_grid_problem(store, labels)
    assert gp.identity and gp.dropout == 'graph'
    chunk = 8192
    batch = mp.web_batch(store, _all_pairs(G, dev), labels.reshape(-1).copy(), batch_total=G * G,
                         chunk=chunk)
    mg.web_grid_fwd_bwd(gp)
    torch.cuda.synchronize()
    gp.check()
    loss_graph = float(mg.loss_buf[0].item())
    assert np.isfinite(loss_graph) and bool(torch.isfinite(mg.grad).all())

    cases = [('web_grid_step_graph_dropout', lambda: mg.web_grid_train_step(gp, sync=False)),
             ('pairwise_step_dropout', lambda: mp.train_step(batch, sync=False)),
             ('web_grid_step_dropout0', lambda: m0.web_grid_train_step(gp0, sync=False))]
    for _, fn in cases:          # warm-up of every shape
        timed(fn, 2)
    ms = {k: [] for k, _ in cases}
    for _ in range(repeats):     # alternated
        for k, fn in cases:
            ms[k].append(timed(fn, iters))
    torch.cuda.synchronize()
    gp.check()
    gp0.check()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    g = med['web_grid_step_graph_dropout']
    _emit(dict(graphs=G, pairs=G * G, D=D, K=K, nodes='200..512', chunk=chunk, dropout=dropout,
               repeats=repeats, iters=iters, loss_graph_dropout=loss_graph, msec=ms,
               msec_median=med, spread_msec={k: max(v) - min(v) for k, v in ms.items()},
               pairwise_over_graph_dropout=med['pairwise_step_dropout'] / g,
               graph_dropout_over_dropout0=g / med['web_grid_step_dropout0'],
               embed_drop_workspace_MB=_lib.web_embed_drop_workspace_bytes(mg.sg, G) / 1e6,
               embed_drop_bwd_workspace_MB=_lib.web_embed_drop_bwd_workspace_bytes(mg.sg, G) / 1e6,
               device=torch.cuda.get_device_name(0), one_box=True))


def main():
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.model_mse import SiameseGCNTNMSE, param_shapes
    if not torch.cuda.is_available():
        raise SystemExit('web_grid_train_bench needs a GPU (there is no CPU fallback)')
    dev = torch.device('cuda', 0)
    G, repeats, iters = _arg('--graphs', 256), _arg('--repeats', 3), _arg('--iters', 3)
    enc, flags, store, labels = _setup(G, 0.0)
    mg = SiameseGCNTNMSE(enc.input_dim(), flags, device=dev, n_max=D)
    mp = SiameseGCNTNMSE(enc.input_dim(), flags, device=dev, n_max=D, params=mg.flat_params())
    assert mg.is_web and mg.sg.keep_prob == 1.0
    gp = mg.web_grid_problem(store, labels)
    assert gp.identity
    pairs = _all_pairs(G, dev)
    chunk = 8192
    batch = mp.web_batch(store, pairs, labels.reshape(-1).copy(), batch_total=G * G, chunk=chunk)

    # same objective: loss and per-variable gradient of (a) against (b)
    mg.web_grid_fwd_bwd(gp)
    mp.fwd_bwd(batch, seed=1)
    torch.cuda.synchronize()
    gp.check()
    la, lb = float(mg.loss_buf[0].item()), float(mp.loss_buf[0].item())
    assert abs(la - lb) <= 1e-4 * max(1.0, abs(lb)), (la, lb)
    ga, gb = mg.grad.cpu().numpy().astype(np.float64), mp.grad.cpu().numpy().astype(np.float64)
    off, rel = 0, {}
    for li, name, shape in param_shapes(mg.layers, enc.input_dim()):
        k = int(np.prod(shape))
        scale = max(float(np.abs(gb[off:off + k]).max()), 1e-30)
        rel['{}.{}'.format(li, name)] = float(np.abs(ga[off:off + k] - gb[off:off + k]).max()) / scale
        off += k
    assert max(rel.values()) <= 1e-4, rel

    sdev, ld = gp.store_dev[1], int(gp.emb.shape[1])

    def a_step():
        mg.web_grid_train_step(gp, sync=False)

    def b_step():
        mp.train_step(batch, seed=1, sync=False)

    def a_embed():
        _lib.web_embed(mg.sg, sdev, gp.uniq, G, mg.params, gp.emb, gp.ws_fwd, gp.status)

    def a_grid():
        _lib.web_score_grid_fwd_bwd(mg.sg, gp.emb, ld, gp.emb, ld, G, G, mg.params, gp.labels, G,
                                    G * G, gp.y_stats, True, None, G, gp.g_q, ld, gp.g_db, ld,
                                    mg.grad, mg.loss_buf, gp.ws_grid)

    def a_sum():
        torch.add(gp.g_q, gp.g_db, out=gp.g_emb)

    def a_embed_bwd():
        _lib.web_embed_bwd(mg.sg, sdev, gp.uniq, G, mg.params, gp.g_emb, ld, mg.grad, gp.ws_embed,
                           gp.status)

    def a_adam():
        mg.apply_adam()

    cases = [('web_grid_step', a_step), ('pairwise_step', b_step), ('web_embed', a_embed),
             ('web_grid_fwd_bwd', a_grid), ('role_sum', a_sum), ('web_embed_bwd', a_embed_bwd),
             ('adam', a_adam)]
    for _, fn in cases:          # warm-up of every shape
        timed(fn, 2)
    ms = {k: [] for k, _ in cases}
    for _ in range(repeats):     # alternated
        for k, fn in cases:
            ms[k].append(timed(fn, iters))
    torch.cuda.synchronize()
    gp.check()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(graphs=G, pairs=G * G, D=D, K=K, nodes='200..512', chunk=chunk, repeats=repeats,
               iters=iters, loss_grid=la, loss_pairwise=lb, max_rel_grad_diff=max(rel.values()),
               msec=ms, msec_median=med, spread_msec={k: max(v) - min(v) for k, v in ms.items()},
               pairwise_over_grid=med['pairwise_step'] / med['web_grid_step'],
               grid_workspace_MB=_lib.web_score_grid_bwd_workspace_bytes(mg.sg, G, G) / 1e6,
               embed_bwd_workspace_MB=_lib.web_embed_bwd_workspace_bytes(mg.sg, G) / 1e6,
               device=torch.cuda.get_device_name(0), one_box=True)
    _emit(res)


if __name__ == '__main__':
    if _arg('--dropout', 0.0) > 0:
        main_dropout(_arg('--dropout', 0.0))
    else:
        main()
