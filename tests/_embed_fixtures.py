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


# ---- float64 reference of the NTN head over given embeddings (test_web_grid_ref.py checks
# it against the oracle; test_gpu_web_grid_shapes.py measures sg_web_score_grid against it)
def ntn_head_ref(e_q, e_db, W, V, bias, U, ntn_mode, K, final_act=None):
    """Scores [m][n] of the NTN head (layers.py:282-310) from embeddings e_q [m][D] (graph 1)
    and e_db [n][D] (graph 2), in float64 from the formula itself:
      m_k = e_i^T W[:,:,k] e_j + V[k] · [e_i, e_j] + bias[k],  r = relu(m),
      s = ΣU · Σ_k r_k  ('reference', quirk A1)  or  Σ_k U_k r_k  ('intended'),
    then final_act (a scalar function such as model.apply_final_act_np) if given.
    W [D][D][K], V [K][2 D], bias [K] or None, U [K] or [K][1].  The contraction over a runs
    as one GEMM [rows][D]·[D][D K] per block of queries; no per-query table in the kernel's
    layout is built."""
    import numpy as np
    e_q = np.asarray(e_q, np.float64)
    e_db = np.asarray(e_db, np.float64)
    W = np.asarray(W, np.float64)
    V = np.asarray(V, np.float64)
    U = np.asarray(U, np.float64).reshape(-1)
    D = W.shape[0]
    assert W.shape == (D, D, K) and V.shape == (K, 2 * D) and U.shape == (K,)
    assert e_q.shape[1] == D and e_db.shape[1] == D
    m, n = e_q.shape[0], e_db.shape[0]
    lin = (e_db @ V[:, D:].T)[:, None, :]                          # V[k][D:] · e_j  [n][1][K]
    lin_q = e_q @ V[:, :D].T                                       # V[k][:D] · e_i  [m][K]
    if bias is not None:
        lin_q = lin_q + np.asarray(bias, np.float64).reshape(1, K)
    Wm = W.reshape(D, D * K)
    out = np.empty((m, n), np.float64)
    blk = max(1, min(256, (1 << 22) // max(1, n * K)))             # [n][blk][K] stays small
    for i0 in range(0, m, blk):
        eb = e_q[i0:i0 + blk]
        t = (eb @ Wm).reshape(-1, D, K)                            # Σ_a e_i[a] W[a][b][k]
        t = np.ascontiguousarray(t.transpose(1, 0, 2)).reshape(D, -1)   # [b][(i, k)]
        mk = (e_db @ t).reshape(n, -1, K) + lin + lin_q[None, i0:i0 + blk, :]
        r = np.maximum(mk, 0.0)
        s = U.sum() * r.sum(axis=2) if ntn_mode == 'reference' else r @ U
        out[i0:i0 + blk] = s.T
    if final_act is not None:
        out = np.array([[float(final_act(float(x))) for x in row] for row in out], np.float64)
    return out


def ntn_head_params(prob):
    """W [D][D][K], V [K][2 D], bias [K] or None, U [K] of the problem's NTN layer, float64
    views of prob.params walked by param_shapes."""
    import numpy as np
    from graphembedding_amd.model_mse import param_shapes
    got, off = {}, 0
    for li, name, shape in param_shapes(prob.layers, prob.d_in):
        size = int(np.prod(shape))
        if prob.layers[li]['kind'] == 'NTN':
            got[name] = prob.params[off:off + size].astype(np.float64).reshape(shape)
        off += size
    assert off == prob.params.size
    return got['weights_W'], got['weights_V'], got.get('bias'), got['weights_U'].reshape(-1)


def signed_embeddings(rows, D, seed, scale=1.0):
    """Synthetic embeddings [rows][D] float32 for the score grid: dense and signed, every
    magnitude in scale · [0.5, 1.5) (second moment about scale²), so no component is so near
    zero that the parameters it multiplies drop out of a score.  Row r depends on (D, seed, r)
    only: a call with fewer rows gives the first rows of a call with more."""
    import numpy as np
    mag = np.random.default_rng([seed, 0]).uniform(0.5, 1.5, size=(rows, D))
    bit = np.random.default_rng([seed, 1]).integers(0, 2, size=(rows, D))
    return (scale * mag * np.where(bit == 1, 1.0, -1.0)).astype(np.float32)


# (D, K, bias, ntn_mode) of every model test_gpu_web_grid_shapes.py scores synthetic
# embeddings with; the seeds follow from them (grid_ref_problem, EMB_SEED).
GRID_REF_MODELS = tuple(
    [(D, 10, True, 'reference') for D in (32, 33, 63, 64, 67, 68, 127, 132, 256, 260, 384, 388)] +
    [(512, 16, True, 'reference'), (63, 16, False, 'reference'), (127, 16, False, 'reference'),
     (260, 10, True, 'intended')])
EMB_SEED = 4242
EMB_SCALE = 1.0   # unit scale meets the sensitivity condition of test_web_grid_ref.py


def grid_ref_embeddings(D, m, n):
    """Query rows [m][D] and database rows [n][D] of the synthetic-embedding grid tests."""
    return (signed_embeddings(m, D, EMB_SEED, EMB_SCALE),
            signed_embeddings(n, D, EMB_SEED + 1, EMB_SCALE))


def grid_ref_problem(D, K, bias=True, ntn_mode='reference'):
    """The dropout-0 graph-store problem whose NTN head the synthetic-embedding grid tests
    use: two graphs (1 and D nodes) only so that the head plan accepts the model."""
    ov = ntn_stack(D, K, 'relu', bias, dropout=0.0, ntn_mode=ntn_mode)
    return sized_problem([1, D], ov, n_max=D, seed=100 + D + K, n_types=60 if D > 400 else 29)


def problem(overrides=None, n_max=10, **kw):
    kw.setdefault('n_graphs', 12)
    kw.setdefault('n_pairs', 4)
    kw.setdefault('n_hi', min(n_max, 10))
    return small_problem(n_max=n_max, flags_overrides=overrides, **kw)
