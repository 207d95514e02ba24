"""The stack zoo (tests/_stack_zoo.py) on the CPU: the oracle that test_gpu_generic_zoo.py
leans on against float64 torch autograd for every entry, the conditions that keep those GPU
comparisons from being vacuous, the host-side kernel path of every entry, and the oracle's
outputs on its earlier seven stacks against values recorded before it learnt the pooled row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _stack_zoo as Z
from oracle import siamese_oracle as O
from test_oracle import _float64_default, torch_loss  # noqa: F401  (autouse float64 fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'oracle_stacks_before_pooled_row.npz')

_CASES = [(n, d) for n in Z.NAMES for d in Z.dropouts(n)]
_IDS = ['{}-drop{}'.format(n, d) for n, d in _CASES]


@pytest.mark.parametrize('name', Z.NAMES)
def test_oracle_matches_torch_autograd(name):
    """test_oracle.py's check and tolerances on every zoo entry, at the entry's dropout."""
    prob = Z.zoo_problem(name)
    spec = prob.oracle_spec()
    g1, g2 = prob.oracle_graphs()
    flat = prob.params.astype(np.float64)
    y = prob.labels.astype(np.float64)
    res = Z.zoo_oracle_step(name)
    s_t, loss_t, grad_t = torch_loss(spec, flat, g1, g2, y, Z.SEED)
    np.testing.assert_allclose(res.s, s_t, rtol=1e-12, atol=1e-12)
    assert abs(res.loss - loss_t) < 1e-10 * max(1, abs(loss_t))
    np.testing.assert_allclose(res.grad, grad_t, rtol=1e-9, atol=1e-11)


def _inspect(prob, seed):
    """Smallest |pre-activation| under a relu (layers, NTN, final activation), and per
    dropout site (layer, side) the kept and dropped element counts over the batch."""
    spec = prob.oracle_spec()
    P = O.unflatten(spec, prob.params.astype(np.float64))
    g1, g2 = prob.oracle_graphs()
    relu_min, sites = np.inf, {}

    def site(li, side, mask):
        k, d = sites.get((li, side), (0, 0))
        sites[(li, side)] = (k + int(np.count_nonzero(mask)), d + int(np.count_nonzero(~mask)))

    for i, (a, b) in enumerate(zip(g1, g2)):
        s, c = O.pair_forward(spec, P, a, b, i, seed)
        for side, caches in enumerate((c['c1'], c['c2'])):
            for lc in caches:
                if lc.get('act') == 'relu':
                    relu_min = min(relu_min, float(np.abs(lc['pre']).min()))
                if spec.layers[lc['li']].get('dropout'):
                    site(lc['li'], side, lc['scale'] != 0 if 'scale' in lc else lc['m'])
        if c['kind'] == 'NTN':
            H = spec.layers[c['hi']]
            if H['inneract'] == 'relu':
                relu_min = min(relu_min, float(np.abs(c['m']).min()))
            if H.get('dropout'):
                site(c['hi'], 0, c['m1'])
                site(c['hi'], 1, c['m2'])
        if spec.final_act == 'relu':
            relu_min = min(relu_min, abs(s))
    return relu_min, sites


@pytest.mark.parametrize('name,dropout', _CASES, ids=_IDS)
def test_zoo_is_not_vacuous(name, dropout):
    """What makes a GPU match on the entry mean something (seeds are chosen so these hold)."""
    prob = Z.zoo_problem(name, dropout)
    spec = prob.oracle_spec()
    res = Z.zoo_oracle_step(name, dropout)
    assert np.ptp(res.s) > 1e-3, 'the scores of the batch are all equal'
    # no variable with a dead gradient (a dead relu would zero a whole layer on both sides)
    gmax = float(np.abs(res.grad_mse).max())
    off = 0
    for li, var, shape in O.param_shapes(spec):
        n = int(np.prod(shape))
        vmax = float(np.abs(res.grad_mse[off:off + n]).max())
        assert vmax >= 1e-6 * gmax, (li, var, vmax, gmax)
        off += n
    # the gradient is far above what fp32 can hold, and most pairs contribute to it: a final
    # activation saturated on the whole batch would leave zeros to compare
    assert gmax >= 1e-3, gmax
    y = prob.labels.astype(np.float64)
    gy = res.yhat - y.mean() if spec.loss_mode == 'broadcast' else (res.yhat - y) / y.size
    live = np.abs(gy * O.final_act_grad(spec, res.s, res.yhat)) > 1e-4
    assert 2 * np.count_nonzero(live) > live.size, (np.count_nonzero(live), live.size)
    if spec.final_act == 'relu':
        assert res.s.min() < 0 < res.s.max(), 'relu final activation: one sign only'
    relu_min, sites = _inspect(prob, Z.SEED)
    # an fp32 sign flip under a relu cannot be what a mismatch is about
    assert relu_min > 1e-5, relu_min
    if dropout > 0:
        assert sites, 'no dropout site'
        for key, (kept, dropped) in sites.items():
            assert kept > 0 and dropped > 0, (key, kept, dropped)
    else:
        assert all(d == 0 for _, d in sites.values())


@pytest.fixture(scope='module')
def L():
    from graphembedding_amd import _lib
    from graphembedding_amd.build import build_hip
    build_hip()
    return _lib.lib()


@pytest.mark.parametrize('name', Z.NAMES)
def test_zoo_entry_is_generic_on_its_own(L, name):
    """Path 0 without SG_DISABLE_FAST, and the oracle's parameter count (host only)."""
    from graphembedding_amd import _lib
    assert 'SG_DISABLE_FAST' not in os.environ
    for dropout in Z.dropouts(name):
        prob = Z.zoo_problem(name, dropout)
        n, path = _lib.validate(Z.lib_model(prob))
        assert path == 0, (name, path)
        assert n == O.n_params(prob.oracle_spec()) == prob.params.size


def test_big_lds_backward_runs_three_waves(L):
    """sg_workspace_bytes sizes the gradient slab with the backward launch's row count,
    ceil(n_pairs / waves per workgroup): at 36 pairs 12 rows for three waves, 9 for four."""
    from graphembedding_amd import _lib
    prob = Z.zoo_problem('big_lds')
    C = prob.params.size + 1

    def ws_bytes(rows):   # siamese_hip.hip: slab rows + 16 reduce partials, 64-float units
        b = ((rows * C + 16 * C + 63) & ~63) * 4
        return max((b + 255) & ~255, (256 + 2) * 8) + 256

    got = _lib.workspace_bytes(Z.lib_model(prob), 36)
    assert got == ws_bytes(12) != ws_bytes(9), (got, ws_bytes(12), ws_bytes(9))


def test_padding_after_pooling_bounds_no_graph():
    """The node-count limit of a store (quirk A9) comes from a Padding layer that pads the
    graph's own rows, not from one that pads the pooled row."""
    from graphembedding_amd.layers_factory import padding_dims
    assert padding_dims(Z.zoo_problem('avg_pad').layers) is None
    assert padding_dims(Z.zoo_problem('att_dense_pad_dot').layers) is None
    assert padding_dims(Z.zoo_problem('three_gcn_pad_wide').layers) == 10
    assert padding_dims(Z.zoo_problem('cap12_pad10').layers) == 10


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import _stack_zoo as Z
want = np.load({golden!r})
got = Z.existing_stack_outputs()
assert sorted(want.files) == sorted(got), (want.files, sorted(got))
bad = [k for k in want.files if not np.array_equal(want[k], got[k])]
for k in bad:
    print(k, float(np.abs(want[k] - got[k]).max()))
sys.exit(1 if bad else 0)
"""


def test_existing_stacks_bit_identical():
    """The pooled-row extension changes nothing for test_oracle.STACKS: scores, losses and
    gradients equal, bit for bit, the values the oracle gave before it.  The bits of a
    float64 matmul or exp depend on the BLAS kernel and the SIMD dispatch numpy picks for
    the CPU at hand, so the comparison runs in a child process that pins both (the
    Haswell OpenBLAS kernels, numpy without AVX-512), as the recording did."""
    env = dict(os.environ, OPENBLAS_NUM_THREADS='1', OPENBLAS_CORETYPE='Haswell',
               NPY_DISABLE_CPU_FEATURES='AVX512F AVX512CD AVX512_KNL AVX512_KNM AVX512_SKX '
                                        'AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR')
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), golden=GOLDEN)
    r = subprocess.run([sys.executable, '-W', 'ignore', '-c', code], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
