"""The problems of test_gpu_fast32_shapes.py (_fast32_cases.py), checked on the references
alone: what a batch must give so that a kernel error in the code it aims at cannot hide.

- No reference score is exactly 0 and no variable's reference gradient is all-zero (or
  1e-6 of the largest variable's: rounding alone), in any batch or sub-batch; most pairs
  score apart from the commonest score, the sign of live embeddings
  (_fast32_cases.check_conditions).
- In the width cases the parameters after Adam can be held to the oracle's on 95 % or more
  of the components (_fast32_cases.adam_well_conditioned).
- The lattice holds every (N0, N1) combination of the kernel's node-count boundaries.
- The one-hot width d_in of the d_in cases is the intended one, and every type occurs.
- Switching one layer's dropout off moves the reference scores by more than 10x the GPU
  tolerance: the switched layer matters to these inputs."""
import numpy as np
import pytest

import _fast32_cases as C

MOVE = 10 * C.TOL


def _check(case):
    ref = C.reference(case)
    C.check_conditions(ref.s, ref.grad_mse, C.problem(case), str(case))
    return ref


@pytest.mark.parametrize('record_dtype', ['f32', 'bf16'])
def test_lattice_covers_every_boundary_pair(record_dtype):
    prob = C.lattice_problem(record_dtype)
    n = np.array([g.number_of_nodes() for g in prob.graphs])
    assert tuple(n) == C.LATTICE_SIZES
    # both sides of every k-block boundary 4 b | 4 b + 1 below D, N = 1 and N = D
    want = {1, C.LATTICE_D} | {m for b in range(1, 8) for m in (4 * b, 4 * b + 1)}
    assert set(C.LATTICE_SIZES) == want
    got = {(int(n[i]), int(n[j])) for i, j in prob.pairs}
    assert got == {(a, b) for a in want for b in want} and len(prob.pairs) == 256
    assert ((prob.labels > 0) & (prob.labels <= 1)).all()
    _check(('lattice', record_dtype))


@pytest.mark.parametrize('k', range(16))
@pytest.mark.parametrize('side', [0, 1])
def test_lattice_sub_batches(side, k):
    prob = C.lattice_sub(side, k)
    assert len(prob.pairs) == 16 and (prob.pairs[:, side] == k).all()
    assert sorted(prob.pairs[:, 1 - side].tolist()) == list(range(16))
    _check(('lattice_sub', side, k))


@pytest.mark.parametrize('D', C.WIDTHS)
def test_width_problems(D):
    cases = [('width', D)] + ([('width', D, True)] if D in C.WIDTH_HEAVY else [])
    for case in cases:
        prob = C.problem(case)
        assert prob.n_max == D and prob.flags.dropout == (0.9 if len(case) == 3 else 0.1)
        n = np.array([g.number_of_nodes() for g in prob.graphs])
        assert {1, 2, D - 1, D} <= set(n.tolist()) and n.max() == D
        assert {m for m in (16, 17) if m <= D} <= set(n.tolist())
        assert set(prob.pairs.ravel().tolist()) == set(range(len(n)))   # every graph is used
        assert (prob.pairs[:, 0] == prob.pairs[:, 1]).sum() >= 6         # self-pairs
        assert (prob.pairs == prob.pairs[0]).all(axis=1).sum() >= 4      # a repeated pair
        ref = _check(case)
        # the parameters after Adam are compared with the oracle's on all but a few
        assert C.adam_well_conditioned(ref, prob).mean() >= 0.95


@pytest.mark.parametrize('d_in', list(C.DIN_CASES))
def test_din_problems(d_in):
    prob = C.din_problem(d_in)
    assert prob.d_in == d_in
    used = set(prob.pairs.ravel().tolist())
    types = np.concatenate([prob.mgs[i].types for i in used])
    assert set(types.tolist()) == set(range(d_in))                       # every type occurs
    n = [g.number_of_nodes() for g in prob.graphs]
    assert min(n) == 1 and max(n) == C.DIN_D
    _check(('din', d_in))


@pytest.mark.parametrize('D', C.MANY_WIDTHS)
def test_many_pairs_problems(D):
    """At the MI355X's 256 compute units (the GPU test sizes the batch by the device's own
    count): 66,305 pairs, so every wave of the 2,048 walks 32 pairs or more."""
    prob = C.many_problem(D)
    n = C.many_pairs_count(C.MANY_CUS)
    assert len(prob.pairs) == n == 66305
    # the weight-gradient kernel's share of block b: pairs n b / 256 .. n (b + 1) / 256
    cut = n * np.arange(C.MANY_CUS + 1) // C.MANY_CUS
    share = np.diff(cut)
    assert set(share.tolist()) == {259, 260} and (share == 259).sum() == C.MANY_CUS - 1
    assert 259 > 2 * 128 and 259 > 4 * 64 and 259 % 4 == 3   # 3 / 5 chunks, a tail of 3
    sizes = np.array([g.number_of_nodes() for g in prob.graphs])
    assert len(sizes) == C.MANY_GRAPHS and set(sizes.tolist()) == set(range(1, D + 1))
    s, g, loss = C.many_reference(D)
    C.check_conditions(s, g, prob, 'many D = {}'.format(D))
    assert np.isfinite(loss)


@pytest.mark.parametrize('stack,layer,only,dropout', C.FLAG_CASES)
def test_dropout_flag_problems(stack, layer, only, dropout):
    prob = C.flag_problem(stack, layer, only, dropout)
    assert prob.flags.dropout == dropout
    switch = {li: L.get('dropout') for li, L in enumerate(prob.layers) if 'dropout' in L}
    assert set(switch) == set(C.FLAG_STACKS[stack][3])
    for li, drops in switch.items():
        assert bool(drops) == ((li != layer) if only == 'off' else (li == layer)), (li, switch)
    ref = _check(('flags', stack, layer, only, dropout))
    if only == 'off':
        on = _check(('flags', stack, None, None, dropout))
        move = float(np.abs(on.s - ref.s).max())
        assert move > MOVE, 'layer {} of {}: all-on scores differ by {:.3g} only'.format(
            layer, stack, move)
