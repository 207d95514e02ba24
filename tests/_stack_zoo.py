"""The stack zoo: small layer stacks that the plan (csrc/sg_plan.h) accepts and no fused
kernel serves, one per branch of the generic kernel (sg_generic.hip, sg_gen_nodes.h) that
the parity stacks of test_gpu_parity.py do not reach.  A plain helper module like
_fixtures.py: the table, the problems built from it and the oracle step of each, computed
once per session and shared by test_stack_zoo_oracle.py (CPU) and test_gpu_generic_zoo.py.

Every entry: 12-16 graphs with explicit node counts (1-node graphs and graphs at the
Padding dim / record capacity among them), 24-48 pairs, widths as small as the branch
allows.  padding_value is an integer: the layer grammar parses it with int(), as the
reference's does (layers_factory.py:98)."""
from __future__ import annotations

import numpy as np

from _embed_fixtures import sized_problem
from oracle import siamese_oracle as O


# ---- layer strings (the grammar of config.py:44-66) -------------------------------------
def gcn(dout, act, din=None, bias=True, dropout=True):
    """GraphConvolution; din=None is the sparse first layer."""
    s = 'GraphConvolution:' + ('' if din is None else 'input_dim={},'.format(din))
    return s + 'output_dim={},act={},dropout={},bias={},sparse_inputs={}'.format(
        dout, act, dropout, bias, din is None)


def dense(din, dout, act, bias=True, dropout=True):
    return 'Dense:input_dim={},output_dim={},dropout={},act={},bias={}'.format(
        din, dout, dropout, act, bias)


def pad(rows, value=0):
    return 'Padding:max_in_dims={},padding_value={}'.format(rows, value)


def ntn(D, K, act, bias=True, dropout=True):
    return 'NTN:input_dim={},feature_map_dim={},inneract={},dropout={},bias={}'.format(
        D, K, act, dropout, bias)


def att(d):
    return 'Attention:input_dim={}'.format(d)


def stack(*layers, **flags):
    ov = dict(num_layers=len(layers))
    for i, s in enumerate(layers):
        ov['layer_{}'.format(i)] = s
    ov.update(flags)
    return ov


# the reference's GCN prefix (config.py:44-52): sparse GCN(d_in -> 32, relu), GCN(32 -> 16, identity)
PREFIX = (gcn(32, 'relu'), gcn(16, 'identity', din=32))
# a narrow prefix for the Dot entries: widths 6 and 5 (no multiple of 4)
NARROW = (gcn(6, 'relu'), gcn(5, 'identity', din=6))

# node counts: two 1-node graphs, two at the capacity, the rest spread between
_C10 = [1, 1, 10, 10, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2]

# The identity final activation of this and of the two padded NTN entries below: their scores
# reach the tens (K = 17 relu maps; pad values times a 40- or 48-wide NTN), where the Gaussian
# exp(-0.6 s^2) underflows and would leave most pairs, at dropout 0.9 all of them, a gradient
# of zero: nothing to compare.  The Gaussian's gradient runs on the entries with small scores.
_DENSE_MID = stack(gcn(6, 'relu'), dense(6, 3, 'sigmoid', bias=False), gcn(4, 'identity', din=3),
                   att(4), ntn(4, 17, 'relu'), final_act='identity')


def _entry(flags, counts=_C10, n_max=10, n_pairs=36, seed=1, n_types=6):
    return dict(flags=flags, counts=list(counts), n_max=n_max, n_pairs=n_pairs, seed=seed,
                n_types=n_types)


ZOO = {
    # GCN rows masked under sigmoid (sigmoid(0) != 0), no-bias GCN, widths 6 / 5 / 3 (alloc
    # rounds every LDS tensor to 4 floats), tanh NTN gradient
    'gcn_sigmoid_tanh_nobias': _entry(stack(
        gcn(6, 'sigmoid', bias=False), gcn(5, 'tanh', din=6), 'Average', ntn(5, 3, 'tanh'))),
    # a third GCN, Padding of a width-4 tensor (D = Pr * width), non-zero pad, identity NTN
    # without bias
    'three_gcn_pad_wide': _entry(stack(
        gcn(8, 'relu'), gcn(6, 'identity', din=8), gcn(4, 'relu', din=6), pad(10, 2),
        ntn(40, 2, 'identity', bias=False), final_act='identity')),
    # Dense before pooling at width > 1 (dropout element r*din + i), no-bias sigmoid Dense,
    # GCN after Dense, K = 17 > one 16-lane group
    'dense_mid_gcn_att_k17': _entry(_DENSE_MID),
    # a negative pad value through an identity Dense of width 2 after Padding, K = 1, sigmoid
    # final activation
    'pad_negative_dense2': _entry(stack(
        *PREFIX, dense(16, 1, 'relu'), pad(10, -1), dense(1, 2, 'identity'), ntn(20, 1, 'relu'),
        final_act='sigmoid')),
    # Dense on the pooled row (R = 1, rin_fixed = 1), K = 64 (the plan's maximum), sigmoid NTN,
    # ntn_mode intended and the aligned loss on a non-fused stack
    'avg_dense_k64': _entry(stack(
        *PREFIX, 'Average', dense(16, 7, 'tanh'), ntn(7, 64, 'sigmoid'),
        ntn_mode='intended', loss_mode='aligned')),
    # Padding of the pooled row (rin_fixed = 1) with a non-zero pad value
    'avg_pad': _entry(stack(*PREFIX, 'Average', pad(3, 2), ntn(48, 2, 'relu'),
                            final_act='identity')),
    # Dense (relu) and Padding after Attention, Dot head on the padded rows
    'att_dense_pad_dot': _entry(stack(
        gcn(6, 'relu'), gcn(4, 'identity', din=6), att(4), dense(4, 3, 'sigmoid'), pad(2, -1),
        'Dot')),
    # bf16 records at odd n_max (n_max^2 = 81 bf16 per side: side 1 starts in the upper half
    # of a word), the widening loop of sg_generic_kernel on a stack that is generic on its
    # own; relu NTN without bias
    'odd_nmax9_bf16': _entry(stack(
        gcn(6, 'relu'), gcn(3, 'tanh', din=6), pad(9), ntn(27, 3, 'relu', bias=False),
        record_dtype='bf16'), counts=[1, 1, 9, 9, 2, 3, 4, 5, 6, 7, 8, 9], n_max=9),
    # f32 records at n_max 7 (record layout at an odd capacity), relu Dense, Dot head on Padding
    'nmax7': _entry(stack(*PREFIX, dense(16, 1, 'relu'), pad(7), 'Dot', final_act='identity'),
                    counts=[1, 1, 7, 7, 2, 3, 4, 5, 6, 7, 5, 3], n_max=7),
    # record capacity 12 above the Padding dim 10 on the pair path; a tanh NTN keeps the
    # default layers off the fused kernels
    'cap12_pad10': _entry(stack(*PREFIX, dense(16, 1, 'relu'), pad(10), ntn(10, 10, 'tanh')),
                          n_max=12),
    # graphs of up to 40 nodes on a stack no fused or graph-store kernel serves: every row
    # loop runs past 32
    'nmax40_average': _entry(stack(
        gcn(8, 'relu'), gcn(4, 'identity', din=8), 'Average', ntn(4, 10, 'relu')),
        counts=[1, 1, 40, 40, 33, 39, 17, 25, 32, 36, 8, 3], n_max=40, n_pairs=24),
    # The backward launch above 64 KB of LDS with three waves, the forward launch with four.
    # sg_build_plan at n_max 16 (floats per wave): record 2*256 + 32 + 4 = 548; GCN0 xd 32,
    # pre 2*16*12 = 384, out 384; GCN1 xd 384, pre 2*16*8 = 256, out 256; Dense xd 256, pre 32,
    # out 32; Padding out 32; NTN x12 32, u 16*12 = 192, m 12, gm 12; four buffers of
    # max_tensor = 2*16*12 = 384.  Sum 4380 floats = 17,520 B.
    # sg_generic_launch, forward: 4 * 17,520 = 70,080 B <= 81,920, so four waves (and the
    # hipFuncSetAttribute branch, 70,080 > 65,536).  Backward: n_params = 12 d_in + 12 + 96 + 8
    # + 8 + 1 + (3072 + 384 + 12 + 12) = 12 d_in + 3605, so the gradient row is at least
    # 3620 floats = 14,480 B (d_in = 1) and at most 3956 floats = 15,824 B (d_in = 29):
    # 4 waves need >= 84,560 B > 81,920, three need 52,560 + [14,480, 15,824] = [67,040,
    # 68,384] B: above 65,536, below 81,920 and below the CU's 163,840 (sg_generic_lds_ok).
    # K = 12 keeps the default layers off the fused capacity-32 kernel.
    'big_lds': _entry(stack(
        gcn(12, 'relu'), gcn(8, 'identity', din=12), dense(8, 1, 'relu'), pad(16),
        ntn(16, 12, 'relu')),
        counts=[1, 1, 16, 16, 2, 5, 9, 11, 13, 15, 16, 7], n_max=16),
    # dense-input dropout indexing with most elements dropped
    'drop90_dense': _entry(dict(_DENSE_MID, dropout=0.9)),
}

# Dot head straight after Average / Attention pooling, every final activation that
# sg_final_grad serves besides the Gaussian and the sigmoid, both loss modes
for _pool in ('average', 'attention'):
    for _fa in ('relu', 'tanh', 'identity'):
        for _lm in ('broadcast', 'aligned'):
            ZOO['dot_{}_{}_{}'.format(_pool, _fa, _lm)] = _entry(stack(
                *NARROW, 'Average' if _pool == 'average' else att(5), 'Dot',
                final_act=_fa, loss_mode=_lm))

NAMES = list(ZOO)
# entries with a layer without bias, for the Adam step
ADAM_NAMES = ('gcn_sigmoid_tanh_nobias', 'three_gcn_pad_wide', 'dense_mid_gcn_att_k17')
SEED = 1234   # dropout seed of every zoo run


def entry_dropout(name):
    """The dropout the entry runs at: its own, else the default of config.py."""
    from graphembedding_amd.config import DEFAULTS
    return ZOO[name]['flags'].get('dropout', DEFAULTS['dropout'])


def dropouts(name):
    """The entry's own dropout and dropout 0."""
    return (entry_dropout(name), 0.0)


_PROBLEMS = {}
_STEPS = {}


def zoo_problem(name, dropout=None):
    """The entry's problem (read only: shared between tests).  Graphs, pairs, labels and
    parameters do not depend on `dropout`."""
    dropout = entry_dropout(name) if dropout is None else dropout
    key = (name, dropout)
    if key not in _PROBLEMS:
        e = ZOO[name]
        prob = sized_problem(e['counts'], dict(e['flags'], dropout=dropout), n_max=e['n_max'],
                             seed=e['seed'], n_types=e['n_types'])
        rng = np.random.default_rng(1000 + e['seed'])
        G, P = len(e['counts']), e['n_pairs']
        pairs = rng.integers(0, G, size=(P, 2)).astype(np.int32)
        # a 1-node graph against one at the capacity in either role, two 1-node graphs, a self-pair
        pairs[:4] = [[0, 2], [3, 1], [0, 1], [2, 2]]
        d = rng.integers(0, 8, size=P)
        nn = np.array([e['counts'][i] + e['counts'][j] for i, j in pairs])
        prob.pairs = pairs
        prob.labels = np.exp(-prob.flags.yeta * (2.0 * d / nn) ** 2).astype(np.float32)
        _PROBLEMS[key] = prob
    return _PROBLEMS[key]


def zoo_oracle_step(name, dropout=None):
    """run_oracle_step of the entry at SEED, computed once."""
    from _fixtures import run_oracle_step
    dropout = entry_dropout(name) if dropout is None else dropout
    key = (name, dropout)
    if key not in _STEPS:
        _STEPS[key] = run_oracle_step(zoo_problem(name, dropout), SEED)
    return _STEPS[key]


def lib_model(prob):
    """The sg_model_t of the problem as SiameseGCNTNMSE builds it (record dtype included)."""
    from graphembedding_amd import _lib
    f = prob.flags
    return _lib.make_model(prob.layers, prob.d_in, prob.n_max, 1.0 - f.dropout, f.final_act,
                           f.sim_kernel, f.yeta, f.loss_mode, f.ntn_mode,
                           getattr(f, 'record_dtype', 'f32') or 'f32')


def existing_stack_outputs():
    """fwd_bwd of the oracle on the seven stacks of test_oracle.STACKS (its problem, its
    seed): {'<stack>.s', '<stack>.loss', '<stack>.grad'} float64 arrays."""
    from _fixtures import small_problem
    from test_oracle import STACKS
    out = {}
    for name, ov in STACKS.items():
        prob = small_problem(n_graphs=8, n_pairs=6, seed=11, flags_overrides=ov)
        g1, g2 = prob.oracle_graphs()
        res = O.fwd_bwd(prob.oracle_spec(), prob.params.astype(np.float64), g1, g2,
                        prob.labels.astype(np.float64), seed=99)
        out[name + '.s'] = res.s
        out[name + '.loss'] = np.array([res.loss, res.loss_mse])
        out[name + '.grad'] = res.grad_mse
    return out
