"""The fused capacity-32 kernel (csrc/sg_fast32.hip, kernel path 2) at every size class,
every Padding / NTN width D, the one-hot width's edges and many pairs per wavefront, and the
per-layer dropout flags of both fused paths — against the numpy oracle (float64) or, for the
~66 k-pair launches, the C restatement (oracle/siamese_cpu.c, gradient summed in double).

The problems and their references come from _fast32_cases.py; test_fast32_cases_ref.py
checks on the CPU that they meet the conditions restated here before each comparison.
Tolerances (north_star): scores 1e-4; gradient 1e-4 of each variable's own largest
reference component; loss 1e-4 relative; bitwise claims by torch.equal."""
import time

import numpy as np
import pytest

import _fast32_cases as C
from _fixtures import check_grad_per_var
from oracle import siamese_oracle as O

pytestmark = pytest.mark.gpu

TOL = C.TOL


def _model(prob, gpu, path=2):
    from graphembedding_amd.model_mse import SiameseGCNTNMSE
    model = SiameseGCNTNMSE(prob.d_in, prob.flags, device=gpu, n_max=prob.n_max,
                            params=prob.params)
    assert model.kernel_path == path, (model.kernel_path, path)
    if path == 2:
        assert model.n_max == 32, model.n_max
    return model


def _batch(model, prob):
    import torch
    from graphembedding_amd.packer import GraphStore
    words = GraphStore(prob.mgs, model.n_max, prob.d_in).pack_host(
        prob.pairs, prob.labels, dtype=model.record_dtype)
    recs = torch.from_numpy(words.view(np.int32).reshape(-1)).to(model.device)
    return model.batch_from_records(recs, len(prob.pairs), prob.labels)


def _check_step(model, prob, ref, what, adam=False):
    """Scores, per-variable gradient and loss of one step on `prob` against `ref`; with
    `adam` also the full loss and the parameters after apply_adam (the model is spent then),
    the latter against the oracle except where C.adam_well_conditioned rules it out."""
    C.check_conditions(ref.s, ref.grad_mse, prob, what)
    batch = _batch(model, prob)
    s = model.pred_sim_without_act(batch, seed=C.ORACLE_SEED).cpu().numpy()
    model.fwd_bwd(batch, seed=C.ORACLE_SEED)
    g = model.grad.cpu().numpy()
    loss_mse = float(model.loss_buf[0].item())
    print('{}: worst |ds| {:.3g}, loss {} vs {}'.format(what, float(np.abs(s - ref.s).max()),
                                                        loss_mse, ref.loss_mse))
    np.testing.assert_allclose(s, ref.s, rtol=TOL, atol=TOL, err_msg=what)
    rel = check_grad_per_var(g, ref.grad_mse, prob.layers, prob.d_in, TOL, what=what)
    print('{}: per-variable relative gradient error {}'.format(what, rel))
    assert abs(loss_mse - ref.loss_mse) <= TOL * max(1.0, abs(ref.loss_mse)), what
    if adam:
        model.apply_adam()
        reg = float(model.reg_buf[0].item())
        assert abs(loss_mse + reg - ref.loss) <= TOL * max(1.0, abs(ref.loss)), what
        new = model.params.cpu().numpy()
        # every parameter: the float64 Adam step on the gradient the kernel left
        p0 = prob.params.astype(np.float64)
        own = O.adam_tf_step(p0, g.astype(np.float64) + prob.flags.weight_decay * p0,
                             O.adam_init(p0.size), lr=prob.flags.learning_rate)
        np.testing.assert_allclose(new, own, rtol=0, atol=C.ADAM_ATOL, err_msg=what)
        # the oracle's step, wherever float32 rounding of the gradient cannot pass the bound
        ok = C.adam_well_conditioned(ref, prob)
        assert ok.mean() >= 0.95, (what, ok.mean())
        print('{}: worst parameter error after Adam {:.3g} ({} of {} compared)'.format(
            what, float(np.abs(new - ref.new_params)[ok].max()), int(ok.sum()), ok.size))
        np.testing.assert_allclose(new[ok], ref.new_params[ok], rtol=0, atol=C.ADAM_ATOL,
                                   err_msg=what)


# ---- 1. the size-class lattice ------------------------------------------------------------
@pytest.fixture(scope='module')
def lattice_model(gpu):
    return _model(C.lattice_problem(), gpu)


@pytest.mark.parametrize('record_dtype', ['f32', 'bf16'])
def test_lattice_all_pairs(gpu, lattice_model, record_dtype):
    """All 256 ordered pairs of the sixteen boundary sizes in one batch: every (T0, T1) tile
    class, k-block count and NTN row class KR next to each other; with bf16 records against
    the oracle on the bf16-rounded Â."""
    prob = C.lattice_problem(record_dtype)
    n = np.array([g.number_of_nodes() for g in prob.graphs])
    assert {(int(n[i]), int(n[j])) for i, j in prob.pairs} == \
        {(a, b) for a in C.LATTICE_SIZES for b in C.LATTICE_SIZES}
    model = lattice_model if record_dtype == 'f32' else _model(prob, gpu)
    assert model.record_dtype == record_dtype
    _check_step(model, prob, C.reference(('lattice', record_dtype)),
                'lattice {}'.format(record_dtype))


@pytest.mark.parametrize('k', range(16), ids=['N{}'.format(n) for n in C.LATTICE_SIZES])
@pytest.mark.parametrize('side', [0, 1], ids=['first', 'second'])
def test_lattice_sub_batch(lattice_model, side, k):
    """The 16 pairs with one graph fixed on one side as a batch of their own: the gradient
    of one size class of that side, not a sum over all of them, so a wrong class fails in
    one 'first' and one 'second' case."""
    case = ('lattice_sub', side, k)
    _check_step(lattice_model, C.problem(case), C.reference(case),
                'lattice, graph {} = {} nodes'.format(side, C.LATTICE_SIZES[k]))


# ---- 2. every width D ---------------------------------------------------------------------
@pytest.mark.parametrize('D', C.WIDTHS)
def test_every_width(gpu, D):
    """D = 13..31: both NTN weight-gradient variants (8 waves of 2 column tiles to D = 16,
    4 waves of 5 from 17) with every count of column tiles and every partial last tile;
    graphs of 1, 2, D − 1 and D nodes, self-pairs and a repeated pair."""
    case = ('width', D)
    prob = C.problem(case)
    assert prob.n_max == D and max(g.number_of_nodes() for g in prob.graphs) == D
    _check_step(_model(prob, gpu), prob, C.reference(case), 'D = {}'.format(D), adam=True)


@pytest.mark.parametrize('D', C.WIDTH_HEAVY)
def test_width_heavy_dropout(gpu, D):
    """Dropout 0.9 at the smallest D of each weight-gradient variant."""
    case = ('width', D, True)
    prob = C.problem(case)
    assert prob.flags.dropout == 0.9
    _check_step(_model(prob, gpu), prob, C.reference(case), 'D = {}, dropout 0.9'.format(D),
                adam=True)


# ---- 3. the one-hot width d_in ------------------------------------------------------------
@pytest.mark.parametrize('d_in', list(C.DIN_CASES))
def test_one_hot_width_edges(gpu, d_in):
    """d_in = 1, 16 | 17 (the type-tile boundary of the one-hot gW0 product) and 32 (the
    zero row at index d_in is the 33rd) at D = 30, every type in use."""
    case = ('din', d_in)
    prob = C.problem(case)
    assert prob.d_in == d_in
    used = np.concatenate([prob.mgs[i].types for i in set(prob.pairs.ravel().tolist())])
    assert set(used.tolist()) == set(range(d_in))
    _check_step(_model(prob, gpu), prob, C.reference(case), 'd_in = {}'.format(d_in))


# ---- 4. many pairs per wave, unsorted classes, multi-chunk weight gradient ----------------
@pytest.mark.parametrize('D', C.MANY_WIDTHS)
def test_many_pairs_per_wave(gpu, D):
    """259 pairs per workgroup (one has 260), drawn uniformly from 60 graphs of 1..D nodes
    and gathered from the dense store: every wave walks about 32 pairs of interleaved size
    classes in batch order (the pair loop's carried state: sT tiles, sX, the ord tables, the
    priority flip), and the NTN weight-gradient reduction runs three chunks of 128 pairs
    (D <= 16) or five of 64 with a last chunk of 3.  Then the same launch in class order."""
    import torch
    from graphembedding_amd.packer import GraphStore
    blocks = torch.cuda.get_device_properties(gpu).multi_processor_count
    t0 = time.perf_counter()
    prob = C.many_problem(D, blocks)
    n = len(prob.pairs)
    assert n == blocks * (2 * 128 + 3) + 1
    s_ref, g_ref, loss_ref = C.many_reference(D, blocks)
    t_ref = time.perf_counter() - t0
    C.check_conditions(s_ref, g_ref, prob, 'many pairs, D = {}'.format(D))
    model = _model(prob, gpu)
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    lab = torch.from_numpy(prob.labels).to(gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    batch = model.batch_from_store(store, n, lab, pair_idx=torch.from_numpy(prob.pairs).to(gpu),
                                   status=status)
    assert abs(float(batch.y_stats[0].item()) - C.label_mean(prob.labels)) <= 6e-8
    model.workspace(n)

    def run():
        s_out = torch.full((n,), float('nan'), dtype=torch.float32, device=gpu)
        model.fwd_bwd(batch, seed=C.MANY_SEED, s_out=s_out, add_label_term=False)
        return s_out, model.grad.clone(), model.loss_buf[:1].clone()

    def check(res, what):
        s = res[0].cpu().numpy()
        loss = float(res[2].item())
        assert not np.isnan(s).any(), '{}: {} scores never written'.format(what,
                                                                          int(np.isnan(s).sum()))
        print('{}: {} pairs, worst |ds| {:.3g}, loss {} vs {}'.format(
            what, n, float(np.abs(s - s_ref).max()), loss, loss_ref))
        np.testing.assert_allclose(s, s_ref, rtol=TOL, atol=TOL, err_msg=what)
        rel = check_grad_per_var(res[1].cpu().numpy(), g_ref, prob.layers, prob.d_in, TOL,
                                 what=what)
        print('{}: per-variable relative gradient error {}'.format(what, rel))
        assert abs(loss - loss_ref) <= TOL * max(1.0, abs(loss_ref)), (what, loss, loss_ref)

    t0 = time.perf_counter()
    first = run()
    check(first, 'D = {}, batch order'.format(D))
    for x, y in zip(first, run()):
        assert torch.equal(x, y), 'a second fwd_bwd differs (batch order)'
    model.balance(batch)
    assert batch.order is not None
    assert np.array_equal(np.sort(batch.order.cpu().numpy()), np.arange(n))
    ordered = run()
    check(ordered, 'D = {}, class order'.format(D))
    assert torch.equal(ordered[0], first[0]), 'class-ordered scores differ from batch order'
    for x, y in zip(ordered, run()):
        assert torch.equal(x, y), 'a second fwd_bwd differs (class order)'
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    print('D = {}: reference {:.2f} s, GPU runs and checks {:.2f} s'.format(
        D, t_ref, time.perf_counter() - t0))


# ---- 5. per-layer dropout flags -----------------------------------------------------------
@pytest.mark.parametrize('stack,layer,only,dropout', C.FLAG_CASES)
def test_per_layer_dropout_flags(gpu, stack, layer, only, dropout):
    """One layer's dropout=False among dropping layers ('off') and one dropping layer among
    the rest ('on'), at dropout 0.1 and 0.5: the per-layer thresholds and the 1 / keep scales
    folded into the kernels' tables (W0 ik0 ik1, b0 ik1, Wd ik2, gW0 ik0, gWd ik2) each
    belong to their own layer.  With all layers on or all off a misplaced scale cancels."""
    path = C.FLAG_STACKS[stack][0]
    case = ('flags', stack, layer, only, dropout)
    prob = C.problem(case)
    drops = {li: bool(L['dropout']) for li, L in enumerate(prob.layers) if 'dropout' in L}
    assert drops == {li: (li != layer) if only == 'off' else (li == layer)
                     for li in C.FLAG_STACKS[stack][3]}
    ref = C.reference(case)
    if only == 'off':   # the switched layer matters to these inputs
        on = C.reference(('flags', stack, None, None, dropout))
        assert float(np.abs(on.s - ref.s).max()) > 10 * TOL
    _check_step(_model(prob, gpu, path), prob, ref,
                '{}: layer {} alone {}, dropout {}'.format(stack, layer, only, dropout))
