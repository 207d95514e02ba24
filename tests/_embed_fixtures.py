"""Problems for the embed-once retrieval tests (include/siamese_embed.h): the default
stack with a chosen Padding / NTN width D, NTN feature_map_dim K, inner activation and
bias, and the stacks of test_gpu_parity."""
from __future__ import annotations

from _fixtures import AVERAGE_STACK, small_problem
from graphembedding_amd import _lib

ATTENTION_STACK = dict(AVERAGE_STACK, layer_2='Attention:input_dim=16')
DENSE_AFTER_PAD = dict(num_layers=6,
                       layer_3='Padding:max_in_dims=10,padding_value=0',
                       layer_4='Dense:input_dim=1,output_dim=1,dropout=True,act=tanh,bias=True',
                       layer_5='NTN:input_dim=10,feature_map_dim=10,inneract=sigmoid,'
                               'dropout=True,bias=False')


def ntn_stack(D=10, K=10, inneract='relu', bias=True, **flags):
    """flags_overrides of the default stack with Padding / NTN width D and K feature maps."""
    ov = dict(layer_3='Padding:max_in_dims={},padding_value=0'.format(D),
              layer_4='NTN:input_dim={},feature_map_dim={},inneract={},dropout=True,'
                      'bias={}'.format(D, K, inneract, bias))
    ov.update(flags)
    return ov


def lib_model(prob, n_max=None, keep_prob=None):
    f = prob.flags
    return _lib.make_model(prob.layers, prob.d_in, n_max or prob.n_max,
                           1.0 - f.dropout if keep_prob is None else keep_prob, f.final_act,
                           f.sim_kernel, f.yeta, f.loss_mode, f.ntn_mode)


def sized_problem(node_counts, overrides=None, n_max=10, seed=5, n_types=29):
    """small_problem with the node count of every graph given (no pairs)."""
    import numpy as np
    from _fixtures import Problem
    from graphembedding_amd.config import Flags
    from graphembedding_amd.data import synthetic_graph
    from graphembedding_amd.graphs import ModelGraph, NodeFeatureOneHotEncoder
    from graphembedding_amd.layers_factory import create_layers
    from graphembedding_amd.model_mse import glorot_flat
    rng = np.random.default_rng(seed)
    graphs = [synthetic_graph(rng, int(n), gid, n_types, p_extra=0.15)
              for gid, n in enumerate(node_counts)]
    enc = NodeFeatureOneHotEncoder(graphs, 'type').pin_sorted()
    mgs = [ModelGraph(g, enc) for g in graphs]
    ov = dict(overrides or {})
    if n_max != 10 and 'layer_3' not in ov and ov.get('num_layers', 5) == 5:
        ov.update(ntn_stack(n_max, 10))
    flags = Flags(**ov)
    d_in = enc.input_dim()
    layers = create_layers(flags, d_in)
    params = glorot_flat(layers, d_in, seed + 1)
    params = params + np.float32(0.05) * rng.standard_normal(params.shape).astype(np.float32)
    return Problem(flags=flags, graphs=graphs, mgs=mgs, d_in=d_in, n_max=n_max,
                   pairs=np.zeros((0, 2), np.int32), labels=np.zeros(0, np.float32),
                   params=params.astype(np.float32), layers=layers)


def oracle_graphs(prob):
    """The oracle's view of the problem's graphs: Â as the f32 store holds it."""
    import numpy as np
    from oracle import siamese_oracle as O
    return [O.Graph(adj=m.adj.astype(np.float32).astype(np.float64), types=m.types)
            for m in prob.mgs]


def gpu_model(prob, device, **flag_overrides):
    from graphembedding_amd.model_mse import SiameseGCNTNMSE
    f = prob.flags.copy(**flag_overrides) if flag_overrides else prob.flags
    return SiameseGCNTNMSE(prob.d_in, f, device=device, n_max=prob.n_max, params=prob.params)


def problem(overrides=None, n_max=10, **kw):
    kw.setdefault('n_graphs', 12)
    kw.setdefault('n_pairs', 4)
    kw.setdefault('n_hi', min(n_max, 10))
    return small_problem(n_max=n_max, flags_overrides=overrides, **kw)
