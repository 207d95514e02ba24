"""Embed-once retrieval, search and training of a Dot-head model against the pair path (GPU only).

    python scripts/dot_grid_bench.py [--repeats 5] [--iters 10] [--out FILE.json]

syn_aids700nef with a GCN -> GCN -> Average -> Dot stack (E = 16) at dropout 0; every case is
timed `--repeats` times, alternated in one process (device events, warmed up), medians reported:
  (a) embed 700 graphs + sg_dot_score_grid 700 x 700, against the pairwise sg_forward over the
      same 490,000 packed records (the generic kernel: the only way the tree filled this matrix
      for a Dot model before; its code is unchanged, so both are timed in one run);
  (b) sg_dot_search_topk against sg_dot_score_grid + sg_topk_rows at 256 x 2^20 synthetic
      embeddings, k = 10 and k = 64, checked bitwise equal before timing;
  (c) AllPairsGrid.train_step against the pairwise AllPairsShard step (forward, backward,
      Adam), loss and per-variable gradient compared before timing.
No ratio is asserted.  Prints one JSON line.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GCN = 'GraphConvolution:{}output_dim={},act={},dropout=True,bias=True,sparse_inputs={}'
STACK = dict(num_layers=4, layer_0=GCN.format('', 32, 'relu', True),
             layer_1=GCN.format('input_dim=32,', 16, 'identity', False), layer_2='Average',
             layer_3='Dot')


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


def main():
    import torch
    from graphembedding_amd.allpairs import AllPairsGrid, AllPairsShard, load_graph_set
    from graphembedding_amd.config import Flags
    from graphembedding_amd.model_mse import SiameseGCNTNMSE, param_shapes
    if not torch.cuda.is_available():
        raise SystemExit('dot_grid_bench needs a GPU (there is no CPU fallback)')
    dev = torch.device('cuda', 0)
    repeats, iters = _arg('--repeats', 5), _arg('--iters', 10)
    flags = Flags(dropout=0.0, **STACK)
    gs = load_graph_set('syn_aids700nef', n_max=10)
    G = len(gs.mgs)
    labels = gs.label_matrix(flags.yeta)
    mg = SiameseGCNTNMSE(gs.d_in, flags, device=dev, n_max=gs.n_max)
    mp = SiameseGCNTNMSE(gs.d_in, flags, device=dev, n_max=gs.n_max, params=mg.flat_params())
    assert mg.is_dot and mg.embed_dim == 16
    grid = AllPairsGrid(gs, labels, dev)
    gp = grid.problem(mg)
    batch = AllPairsShard(gs, labels, device=dev).batch(mp)

    # (a) the same matrix both ways
    s_grid = mg.score_grid(mg.embed(gs.store), mg.embed(gs.store), final=False)
    s_pair = mp.pred_sim_without_act(batch, seed=1).reshape(G, G)
    score_diff = float((s_grid - s_pair).abs().max().item())
    assert score_diff <= 1e-4 * max(1.0, float(s_pair.abs().max().item())), score_diff

    # (c) the same objective: loss and per-variable gradient
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

    # (b) 256 queries against 2^20 synthetic database rows
    M, N, E = 256, 1 << 20, mg.embed_dim
    rng = np.random.default_rng(0)
    q = torch.from_numpy(rng.standard_normal((M, E)).astype(np.float32)).to(dev)
    db = torch.from_numpy(rng.standard_normal((N, E)).astype(np.float32)).to(dev)
    for k in (10, 64):
        ti, tv = mg.topk(mg.score_grid(q, db), k)
        si, sv = mg.search(q, db, k)
        assert torch.equal(ti, si) and torch.equal(tv.view(torch.int32), sv.view(torch.int32)), k
    del ti, tv, si, sv

    def a_embed_grid():
        e = mg.embed(gs.store)
        mg.score_grid(e, e, final=False)

    def a_pairs():
        mp.pred_sim_without_act(batch, seed=1)

    def b_two_call(k):
        return lambda: mg.topk(mg.score_grid(q, db), k)

    def b_search(k):
        return lambda: mg.search(q, db, k)

    cases = [('embed_grid_700', a_embed_grid, iters), ('pair_forward_700', a_pairs, 2),
             ('grid_topk_k10', b_two_call(10), 2), ('search_k10', b_search(10), iters),
             ('grid_topk_k64', b_two_call(64), 2), ('search_k64', b_search(64), iters),
             ('grid_step_700', lambda: grid.train_step(mg, sync=False), iters),
             ('pairwise_step_700', lambda: mp.fwd_bwd_adam(batch, seed=1), 2)]
    for _, fn, _ in cases:       # warm-up of every shape
        timed(fn, 1)
    ms = {k: [] for k, _, _ in cases}
    for _ in range(repeats):     # alternated
        for k, fn, it in cases:
            ms[k].append(timed(fn, it))
    torch.cuda.synchronize()
    gp.check()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(graphs=G, pairs=G * G, embed_dim=E, search_shape=[M, N], repeats=repeats,
               iters=iters, max_score_diff=score_diff, loss_grid=la, loss_pairwise=lb,
               max_rel_grad_diff=max(rel.values()), msec=ms, msec_median=med,
               spread_msec={k: max(v) - min(v) for k, v in ms.items()},
               pair_forward_over_embed_grid=med['pair_forward_700'] / med['embed_grid_700'],
               grid_topk_over_search_k10=med['grid_topk_k10'] / med['search_k10'],
               grid_topk_over_search_k64=med['grid_topk_k64'] / med['search_k64'],
               pairwise_step_over_grid_step=med['pairwise_step_700'] / med['grid_step_700'],
               device=torch.cuda.get_device_name(0), one_box=True)
    line = json.dumps(res)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
