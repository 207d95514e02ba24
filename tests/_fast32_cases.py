"""Problems for the capacity-32 fused kernel's shape tests (csrc/sg_fast32.hip, kernel path
2) and for the per-layer dropout flags of both fused paths, with their references.

Every problem is a _fixtures.Problem built from a fixed seed; `reference(case)` is the numpy
oracle's step on it (float64), computed once per process and returned read-only, so
test_gpu_fast32_shapes.py (the kernels) and test_fast32_cases_ref.py (the conditions the
problems must meet, on the oracle alone) see the same numbers.  The many-pairs problems are
checked by the C restatement (oracle/siamese_cpu.c, gradient summed in double) instead.

The seeds were picked so that the reference alone meets the conditions of
test_fast32_cases_ref.py: no case is filtered or skipped to make them hold."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from _embed_fixtures import ATTENTION_STACK, ntn_stack, sized_problem
from _fixtures import AVERAGE_STACK, _check_pairs, run_oracle_step
from graphembedding_amd.config import Flags
from graphembedding_amd.packer import GraphStore

TOL = 1e-4
ORACLE_SEED = 777           # dropout seed of every oracle-checked case


def with_pairs(prob, pairs, labels):
    return dataclasses.replace(prob, pairs=np.ascontiguousarray(pairs, np.int32),
                               labels=np.ascontiguousarray(labels, np.float32))


def uniform_labels(n, seed):
    """Labels uniform in (0, 1)."""
    return (1.0 - np.random.default_rng([seed, 99]).random(n)).astype(np.float32)


def _frozen(ref):
    for v in vars(ref).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- 1. the size-class lattice (D = 31) ---------------------------------------------------
# both sides of every node-count boundary of the kernel: the tile class (N > 16), the k-blocks
# of 4 nodes, the NTN row class KR (k-blocks of side 0 in pairs) and D itself
LATTICE_SIZES = (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 31)
LATTICE_D = 31
LATTICE_SEED = 5


@functools.lru_cache(maxsize=None)
def lattice_problem(record_dtype='f32'):
    """All 256 ordered pairs of sixteen graphs with the LATTICE_SIZES node counts; pair
    16 i + j is (graph i, graph j)."""
    ov = dict(dropout=0.1)
    if record_dtype != 'f32':
        ov['record_dtype'] = record_dtype
    prob = sized_problem(LATTICE_SIZES, ov, n_max=LATTICE_D, seed=LATTICE_SEED)
    G = len(LATTICE_SIZES)
    i, j = np.divmod(np.arange(G * G), G)
    return with_pairs(prob, np.stack([i, j], axis=1), uniform_labels(G * G, LATTICE_SEED))


def lattice_sub(side, k):
    """The 16 pairs of the lattice whose graph on `side` (0 / 1) is graph k, as a batch of
    its own (pair keys 0..15)."""
    prob = lattice_problem()
    idx = np.flatnonzero(prob.pairs[:, side] == k)
    return with_pairs(prob, prob.pairs[idx], prob.labels[idx])


# ---- 2. every Padding / NTN width D -------------------------------------------------------
WIDTHS = tuple(range(13, 32))
WIDTH_HEAVY = (13, 17)      # the smallest D of each NTN weight-gradient variant, dropout 0.9
WIDTH_PAIRS = 40
WIDTH_SEEDS = {13: 113, 14: 214, 15: 115, 16: 116, 17: 117, 18: 118, 19: 419, 20: 120, 21: 321,
               22: 222, 23: 123, 24: 124, 25: 225, 26: 126, 27: 127, 28: 328, 29: 229, 30: 230,
               31: 131}
WIDTH_HEAVY_SEEDS = {13: 413, 17: 517}


@functools.lru_cache(maxsize=None)
def width_problem(D, heavy=False):
    """Graphs of 1, 2, D − 1, D nodes, 16 and 17 where they fit, and four random sizes; 40
    pairs that use every graph, with six self-pairs and one pair three times."""
    seed = (WIDTH_HEAVY_SEEDS if heavy else WIDTH_SEEDS)[D]
    rng = np.random.default_rng([seed, 1])
    sizes = [1, 2, D - 1, D] + [n for n in (16, 17) if n < D - 1]
    sizes += [int(n) for n in rng.integers(3, D - 1, size=4)]
    prob = sized_problem(sizes, dict(dropout=0.9 if heavy else 0.1), n_max=D, seed=seed)
    G = len(sizes)
    pairs = rng.integers(0, G, size=(WIDTH_PAIRS, 2))
    pairs[:G, 0] = rng.permutation(G)           # every graph on side 0 ...
    pairs[G:2 * G, 1] = rng.permutation(G)      # ... and on side 1
    pairs[2 * G:2 * G + 6, 1] = pairs[2 * G:2 * G + 6, 0]
    pairs[-3:] = pairs[0]
    return with_pairs(prob, pairs, uniform_labels(WIDTH_PAIRS, seed))


# ---- 3. the one-hot width d_in on path 2 (D = 30) -----------------------------------------
DIN_D = 30
# d_in: (n_types, graphs, seed) — graphs enough that every one of the Zipf-drawn types occurs
DIN_CASES = {1: (1, 12, 301), 16: (16, 60, 316), 17: (17, 60, 317), 32: (32, 160, 332)}


@functools.lru_cache(maxsize=None)
def din_problem(d_in):
    n_types, G, seed = DIN_CASES[d_in]
    rng = np.random.default_rng([seed, 1])
    sizes = [1, DIN_D] + [int(n) for n in rng.integers(2, DIN_D + 1, size=G - 2)]
    prob = sized_problem(sizes, dict(dropout=0.1), n_max=DIN_D, seed=seed, n_types=n_types)
    # every graph once on each side, so every type's W0 row takes a gradient
    pairs = np.stack([np.arange(G), rng.permutation(G)], axis=1)
    return with_pairs(prob, pairs, uniform_labels(G, seed))


# ---- 4. many pairs per wave, classes interleaved, multi-chunk weight gradient ---------------
MANY_WIDTHS = (13, 16, 17)
MANY_GRAPHS = 60
MANY_SEED = 4242            # the launch's dropout seed
MANY_CUS = 256              # the compute units of an MI355X (the CPU module's batch size)
MANY_SEEDS = {13: 613, 16: 416, 17: 717}


def many_pairs_count(blocks):
    """Pairs that give each of `blocks` workgroups 2 · 128 + 3 (and one of them one more):
    three chunks of the 8-wave weight-gradient kernel, five of the 4-wave one, the last
    chunk no multiple of 4 pairs."""
    return blocks * (2 * 128 + 3) + 1


@functools.lru_cache(maxsize=None)
def many_problem(D, blocks=MANY_CUS):
    """About 60 graphs of 1..D nodes (every size at least once) and pairs drawn uniformly
    from them, in drawing order."""
    seed = MANY_SEEDS[D]
    rng = np.random.default_rng([seed, 1])
    sizes = list(range(1, D + 1))
    sizes += [int(n) for n in rng.integers(1, D + 1, size=MANY_GRAPHS - len(sizes))]
    prob = sized_problem(sizes, dict(dropout=0.1), n_max=D, seed=seed)
    n = many_pairs_count(blocks)
    pairs = rng.integers(0, len(sizes), size=(n, 2))
    return with_pairs(prob, pairs, uniform_labels(n, seed))


def label_mean(labels):
    """ȳ as the model's batches hold it: the float64 mean, rounded to float32."""
    return float(np.float32(np.asarray(labels, np.float64).mean()))


@functools.lru_cache(maxsize=None)
def many_reference(D, blocks=MANY_CUS):
    """(scores, gradient, loss) of the C restatement at record capacity D over the pairs of
    many_problem, keys 0..n-1, without the label term of the loss."""
    prob = many_problem(D, blocks)
    f = prob.flags
    s, g, loss = _check_pairs(GraphStore(prob.mgs, D, prob.d_in), prob.pairs, prob.labels, D,
                              prob.d_in, prob.params, MANY_SEED, 1.0 - f.dropout, f.yeta,
                              label_mean(prob.labels), 0, 16384)
    s.setflags(write=False)
    g.setflags(write=False)
    return s, g, loss


# ---- 5. per-layer dropout flags on both fused paths ---------------------------------------
def _stack_layers(ov):
    f = Flags(**ov)
    return {'layer_{}'.format(i): getattr(f, 'layer_{}'.format(i)) for i in range(f.num_layers)}


# stack: (kernel path, Padding / NTN capacity n_max, flag overrides, switchable layers)
FLAG_STACKS = {
    'c4': (2, 30, ntn_stack(30), (0, 1, 2, 4)),
    'default': (1, 10, {}, (0, 1, 2, 4)),
    'average': (1, 10, AVERAGE_STACK, (0, 1, 3)),
    'attention': (1, 10, ATTENTION_STACK, (0, 1, 3)),
}
FLAG_DROPOUTS = (0.1, 0.5)
FLAG_SEEDS = {'c4': 502, 'default': 506, 'average': 500, 'attention': 500}
FLAG_CASES = tuple((stack, layer, only, dropout)
                   for stack, (_, _, _, layers) in FLAG_STACKS.items()
                   for layer in layers for only in ('off', 'on') for dropout in FLAG_DROPOUTS)


@functools.lru_cache(maxsize=None)
def flag_problem(stack, layer=None, only=None, dropout=0.1):
    """16 graphs, 40 pairs on `stack`; only='off': layer `layer` alone has dropout=False,
    only='on': it alone has dropout=True; layer None: every layer drops."""
    _, n_max, ov, layers = FLAG_STACKS[stack]
    spec = _stack_layers(ov)
    for li in layers:
        assert 'dropout=True' in spec['layer_{}'.format(li)], (stack, li)
        drops = True if layer is None else (li != layer) if only == 'off' else (li == layer)
        if not drops:
            key = 'layer_{}'.format(li)
            spec[key] = spec[key].replace('dropout=True', 'dropout=False')
    seed = FLAG_SEEDS[stack]
    rng = np.random.default_rng([seed, 1])
    sizes = [1, n_max] + [int(n) for n in rng.integers(2, n_max + 1, size=14)]
    prob = sized_problem(sizes, dict(ov, dropout=dropout, **spec), n_max=n_max, seed=seed)
    pairs = rng.integers(0, len(sizes), size=(40, 2))
    pairs[:16, 0] = rng.permutation(16)
    return with_pairs(prob, pairs, uniform_labels(40, seed))


# ---- references ---------------------------------------------------------------------------
_BUILDERS = {'lattice': lattice_problem, 'lattice_sub': lattice_sub, 'width': width_problem,
             'din': din_problem, 'flags': flag_problem}


def problem(case):
    """case = (group, *arguments of the group's builder)."""
    return _BUILDERS[case[0]](*case[1:])


@functools.lru_cache(maxsize=None)
def reference(case):
    """The numpy oracle's step (scores, loss, gradient, parameters after Adam) on the case."""
    return _frozen(run_oracle_step(problem(case), ORACLE_SEED))


def _param_shapes(prob):
    from graphembedding_amd.model_mse import param_shapes
    return param_shapes(prob.layers, prob.d_in)


def variable_maxima(grad, prob):
    """{variable: largest |component|} of a flat gradient."""
    g = np.abs(np.asarray(grad, np.float64).reshape(-1))
    out, off = {}, 0
    for li, name, shape in _param_shapes(prob):
        n = int(np.prod(shape))
        out['{}.{}'.format(li, name)] = float(g[off:off + n].max())
        off += n
    assert off == g.size
    return out


def live_share(s_ref):
    """The share of scores that differ from the most frequent score.  A graph whose Dense
    relu is dead at every node embeds to zero, and pairs of such graphs all score the NTN
    bias term alone: they measure nothing of the kernel's NTN products."""
    _, counts = np.unique(np.asarray(s_ref, np.float64), return_counts=True)
    return 1.0 - counts.max() / float(np.asarray(s_ref).size)


def live_min(prob):
    """The live share asked of a batch: 0.8, and 0.5 from dropout 0.5 on, where whole
    embeddings are dropped by design."""
    return 0.8 if prob.flags.dropout < 0.5 else 0.5


ADAM_ATOL = 2e-5            # parameters after the first Adam step (test_gpu_fast32.py)


def adam_well_conditioned(ref, prob):
    """Mask of the parameters whose first Adam step can be compared with the oracle's.

    The first TF-form step moves a parameter by lr · g / (|g| + c), c = eps / sqrt(1 − β2) =
    3.2e-7, with g = ∂loss_mse/∂θ + weight_decay · θ: an error δ in g moves the new parameter
    by lr · c · δ / (|g| + c)², up to 3.2e4 · δ where the two terms of g cancel.  A float32
    gradient carries a rounding error of the order of 32 ulp of its variable's largest
    component M (1.9e-6 · M, fifty times below the gradient tolerance); where that alone
    moves the parameter by more than half of ADAM_ATOL, no float32 kernel can be held to the
    oracle's value, and the test compares such a parameter with the float64 Adam step on the
    kernel's own gradient instead.  About 1 % of the parameters."""
    lr = prob.flags.learning_rate
    c = 1e-8 / np.sqrt(1.0 - 0.999)
    sens = lr * c / (np.abs(ref.grad) + c) ** 2
    big = variable_maxima(ref.grad_mse, prob)
    M = np.concatenate([np.full(int(np.prod(shape)), big['{}.{}'.format(li, name)])
                        for li, name, shape in _param_shapes(prob)])
    # (a component the oracle leaves exactly 0 carries no rounding: it stays compared)
    return (ref.grad_mse == 0.0) | (sens * (32 * 2.0 ** -24 * M) <= 0.5 * ADAM_ATOL)


def check_conditions(s_ref, g_ref, prob, what):
    """What every batch here must give on the reference alone: no score exactly 0 (a dead
    NTN head hides the whole pair), no variable with an all-zero gradient (its kernel
    code would go unmeasured), and mostly live embeddings (live_share)."""
    s_ref = np.asarray(s_ref)
    assert live_share(s_ref) >= live_min(prob), (what, live_share(s_ref))
    assert s_ref.shape[0] == len(prob.pairs) and np.isfinite(s_ref).all(), what
    dead = np.flatnonzero(s_ref == 0.0)
    assert dead.size == 0, '{}: reference scores exactly 0 at pairs {}'.format(what, dead[:8])
    big = variable_maxima(g_ref, prob)
    floor = 1e-6 * max(big.values())    # an all-zero gradient, or one that is rounding alone
    zero = [k for k, v in big.items() if v <= floor]
    assert not zero, '{}: all-zero reference gradient of {}'.format(what, zero)
