"""The generic pair kernel (sg_generic.hip, sg_gen_nodes.h) and the embed-once kernels that
share its node stack (sg_embed.hip, sg_embed_train.hip) against the float64 oracle on the
stack zoo (tests/_stack_zoo.py): every layer option sg_build_plan accepts that the parity
stacks do not reach, each entry generic on its own (kernel path 0 without SG_DISABLE_FAST).
test_stack_zoo_oracle.py checks the oracle itself, and that a match here is not vacuous.
Tolerance: the project's 1e-4 (test_gpu_parity.TOL), rtol = atol; Adam atol 2e-5.
The gradient is not asserted bitwise reproducible: the kernel sums it with LDS float atomics."""
import numpy as np
import pytest

import _stack_zoo as Z
from _embed_fixtures import gpu_model
from _fixtures import check_grad_per_var
from test_gpu_embed import _oracle_embeddings
from test_gpu_embed_train import (SENTINEL, _check_node_range, _oracle_embed_bwd,
                                  _run_embed_bwd)

pytestmark = pytest.mark.gpu

TOL = 1e-4

_CASES = [(n, d) for n in Z.NAMES for d in Z.dropouts(n)]
_IDS = ['{}-drop{}'.format(n, d) for n, d in _CASES]


def _model(prob, gpu):
    model, batch = prob.make_gpu_model(device=gpu)
    assert model.kernel_path == 0, 'the entry must be generic on its own'
    assert model.n_max == prob.n_max   # no switch to a fused kernel's record capacity
    return model, batch


@pytest.mark.parametrize('name,dropout', _CASES, ids=_IDS)
def test_zoo_step_matches_oracle(gpu, name, dropout):
    """Scores, per-variable gradient and loss at the entry's dropout and at dropout 0; one
    Adam step for the entries with a layer without bias."""
    import torch
    prob = Z.zoo_problem(name, dropout)
    model, batch = _model(prob, gpu)
    ref = Z.zoo_oracle_step(name, dropout)
    s_fwd = model.pred_sim_without_act(batch, seed=Z.SEED)
    s = s_fwd.cpu().numpy()
    print('{} dropout {}: max |s - oracle| {:.3g} (max |s| {:.3g})'.format(
        name, dropout, float(np.abs(s - ref.s).max()), float(np.abs(ref.s).max())))
    np.testing.assert_allclose(s, ref.s, rtol=TOL, atol=TOL)
    s_bwd = torch.full_like(s_fwd, -7.25)
    model.fwd_bwd(batch, seed=Z.SEED, s_out=s_bwd)
    g = model.grad.cpu().numpy()
    ref_max = np.abs(ref.grad_mse).max()
    print('  gradient error / largest reference component, whole vector: {:.3g}'.format(
        float(np.abs(g - ref.grad_mse).max() / ref_max)))
    rel = check_grad_per_var(g, ref.grad_mse, prob.layers, prob.d_in, TOL, name)
    print('  per variable:', {k: float('{:.3g}'.format(v)) for k, v in rel.items()})
    loss_mse = float(model.loss_buf[0].item())
    print('  loss {:.8g} oracle {:.8g}'.format(loss_mse, ref.loss_mse))
    assert abs(loss_mse - ref.loss_mse) <= TOL * max(1.0, abs(ref.loss_mse))
    np.testing.assert_allclose(s_bwd.cpu().numpy(), ref.s, rtol=TOL, atol=TOL)
    if name == 'big_lds':
        # three waves per workgroup backward, four forward: the per-pair math must not differ
        assert torch.equal(s_bwd, s_fwd)
    if name in Z.ADAM_NAMES:
        model.apply_adam()
        reg = float(model.reg_buf[0].item())
        assert abs(loss_mse + reg - ref.loss) <= TOL * max(1.0, abs(ref.loss))
        np.testing.assert_allclose(model.params.cpu().numpy(), ref.new_params, rtol=0, atol=2e-5)


@pytest.mark.parametrize('name', Z.NAMES)
def test_zoo_split_forward_is_bitwise(gpu, name):
    """The forward of the batch split at an odd index equals the unsplit forward bit for bit
    (pair_offset keys the dropout masks, batch_total the loss)."""
    prob = Z.zoo_problem(name)
    model, batch = _model(prob, gpu)
    s_full = model.pred_sim_without_act(batch, seed=Z.SEED).cpu().numpy()
    cut = 13
    assert 0 < cut < batch.n_pairs
    W = batch.records.numel() // batch.n_pairs
    b0 = model.batch_from_records(batch.records[:cut * W], cut, batch.labels[:cut], 0,
                                  batch.n_pairs, y_stats=batch.y_stats)
    b1 = model.batch_from_records(batch.records[cut * W:], batch.n_pairs - cut,
                                  batch.labels[cut:], cut, batch.n_pairs, y_stats=batch.y_stats)
    s0 = model.pred_sim_without_act(b0, seed=Z.SEED).cpu().numpy()
    s1 = model.pred_sim_without_act(b1, seed=Z.SEED).cpu().numpy()
    assert np.array_equal(np.concatenate([s0, s1]), s_full)


# ---- embed-once on the same stacks, dropout 0 -------------------------------------------
@pytest.mark.parametrize('name', Z.NAMES)
def test_zoo_embeddings_and_node_backward_match_oracle(gpu, name):
    """model.embed against O._node_forward and sg_embed_bwd with a random upstream gradient
    against O._node_backward, per variable (every zoo entry has sg_embed_dim >= 0: none is on
    the graph-store path)."""
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import GraphStore
    prob = Z.zoo_problem(name, 0.0)
    model = gpu_model(prob, gpu)
    assert model.kernel_path == 0 and model.n_max == prob.n_max
    assert _lib.embed_dim(model.sg) >= 0           # raises for a model without the kernel
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    ref = _oracle_embeddings(prob)
    assert model.embed_dim == ref.shape[1]
    emb = model.embed(store).cpu().numpy()
    print('{}: max |emb - oracle| {:.3g}'.format(name, float(np.abs(emb - ref).max())))
    np.testing.assert_allclose(emb, ref, rtol=TOL, atol=TOL)
    rng = np.random.default_rng(17)
    G = len(store)
    idx = rng.integers(0, G, size=9)        # an odd tail, repeats
    idx[:4] = rng.permutation(4)            # the 1-node graphs and the graphs at the capacity
    idx[-1] = idx[0]
    g_emb = rng.standard_normal((len(idx), model.embed_dim)).astype(np.float32)
    got, st = _run_embed_bwd(model, store.to_device(gpu), idx, g_emb)
    assert st == 0
    _check_node_range(prob, got, _oracle_embed_bwd(prob, idx, g_emb))


@pytest.mark.parametrize('name', Z.NAMES)
def test_zoo_documented_refusals(gpu, name):
    """include/siamese_embed_train.h: sg_embed_bwd refuses a model with effective dropout
    (SG_ERR_UNSUPPORTED) and writes nothing.  include/siamese_embed.h: the score grid serves
    the NTN head with D <= 31 and feature_map_dim <= 16 and refuses the Dot head and larger
    heads with SG_ERR_UNSUPPORTED (workspace size -1)."""
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import GraphStore
    prob = Z.zoo_problem(name)                      # the entry's own dropout: > 0
    assert prob.flags.dropout > 0
    model = gpu_model(prob, gpu)
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    dev = store.to_device(gpu)
    E = model.embed_dim
    with pytest.raises(_lib.SiameseHipError, match='dropout'):   # the size query gives -1
        _lib.embed_bwd_workspace_bytes(model.sg, 4)
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=gpu)
    ws = torch.zeros(1 << 16, dtype=torch.float32, device=gpu)
    g_emb = torch.ones((4, E), dtype=torch.float32, device=gpu)
    with pytest.raises(_lib.SiameseHipError, match='SG_ERR_UNSUPPORTED'):
        _lib.embed_bwd(model.sg, dev, model.n_max, None, 4, model.params, g_emb, grad, ws)
    torch.cuda.synchronize()
    assert bool((grad == SENTINEL).all())
    H = prob.layers[-1]
    served = H['kind'] == 'NTN' and H['input_dim'] <= 31 and H['feature_map_dim'] <= 16
    if served:
        assert _lib.score_grid_workspace_bytes(model.sg, 4) > 0
        return
    with pytest.raises(_lib.SiameseHipError, match='input_dim <= 31'):   # the size query gives -1
        _lib.score_grid_workspace_bytes(model.sg, 4)
    e = torch.zeros((4, E), dtype=torch.float32, device=gpu)
    out = torch.full((4, 4), SENTINEL, dtype=torch.float32, device=gpu)
    with pytest.raises(_lib.SiameseHipError, match='SG_ERR_UNSUPPORTED'):
        _lib.score_grid(model.sg, e, e, 4, 4, model.params, False, out, 4, ws)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
