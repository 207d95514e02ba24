"""Embed-once training on the GPU (include/siamese_embed_train.h): the NTN grid's forward,
loss and adjoint against float64 torch autograd, its bitwise determinism, the node-stack
backward against the oracle's _node_backward, and grid_fwd_bwd / grid_train_step end to end
against the pairwise path (sg_fwd_bwd_src) and the oracle.
Bars are the project's: scores and loss within 1e-4 (rtol = atol, test_gpu_parity.TOL), every
gradient block within 1e-4 of its own largest component (_fixtures.check_grad_per_var).
Three free-running Adam steps are held to the 1e-4 the trajectory test asserts on its
free-running parameters."""
import numpy as np
import pytest

from _embed_fixtures import (ATTENTION_STACK, DENSE_AFTER_PAD, gpu_model, ntn_stack,
                             oracle_graphs, sized_problem)
from _fixtures import AVERAGE_STACK, check_grad_per_var
from oracle import siamese_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -7.25


def _offsets(prob):
    """{(layer, variable): (offset, shape)} of the flat parameter vector, and its size."""
    from graphembedding_amd.model_mse import param_shapes
    off, out = 0, {}
    for li, name, shape in param_shapes(prob.layers, prob.d_in):
        out[(li, name)] = (off, shape)
        off += int(np.prod(shape))
    return out, off


def _block_close(got, want, what):
    """max |got - want| <= TOL x the block's own largest |want| (floored like
    check_grad_per_var so an all-zero block does not divide by zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    print('{}: rel err {:.3g} (scale {:.3g})'.format(what, err, scale))
    assert err <= TOL, (what, err, scale)


# ---- 1. the grid's adjoint against autograd ---------------------------------------------
# (D, K, m, n, ntn_mode, loss_mode, inneract, bias, final): D covers every k-step count's
# edge and the b == D row landing in a second 16-row tile (16, 31); K the one-column, the
# masked (10 of 16) and the full tile; n one row, one block less one, a full block, one
# more, three blocks; m fewer queries than wavefronts, one per wavefront, a second round,
# several chunks.
GRID_CASES = [
    (3, 1, 1, 1, 'reference', 'broadcast', 'relu', True, 'gaussian'),
    (3, 10, 4, 63, 'intended', 'aligned', 'sigmoid', False, 'gaussian'),
    (3, 16, 5, 64, 'reference', 'aligned', 'tanh', True, 'identity'),
    (3, 10, 9, 130, 'reference', 'broadcast', 'identity', True, 'tanh'),
    (10, 1, 9, 65, 'intended', 'broadcast', 'identity', False, 'sigmoid'),
    (10, 10, 9, 130, 'reference', 'broadcast', 'relu', True, 'gaussian'),
    (10, 10, 5, 65, 'intended', 'broadcast', 'relu', True, 'gaussian'),
    (10, 10, 9, 63, 'reference', 'aligned', 'relu', True, 'gaussian'),
    (10, 10, 4, 64, 'reference', 'broadcast', 'sigmoid', False, 'gaussian'),
    (10, 10, 1, 64, 'intended', 'aligned', 'tanh', False, 'relu'),
    (10, 16, 4, 130, 'reference', 'aligned', 'sigmoid', True, 'tanh'),
    (11, 1, 5, 130, 'reference', 'aligned', 'relu', False, 'gaussian'),
    (11, 10, 9, 1, 'intended', 'broadcast', 'sigmoid', True, 'identity'),
    (11, 16, 4, 65, 'reference', 'broadcast', 'identity', True, 'relu'),
    (16, 1, 4, 64, 'intended', 'aligned', 'sigmoid', True, 'sigmoid'),
    (16, 10, 5, 63, 'reference', 'broadcast', 'tanh', False, 'tanh'),
    (16, 10, 1, 65, 'reference', 'aligned', 'identity', True, 'gaussian'),
    (16, 16, 9, 130, 'intended', 'broadcast', 'relu', True, 'gaussian'),
    (16, 16, 5, 1, 'intended', 'aligned', 'relu', False, 'gaussian'),
    (31, 1, 9, 63, 'reference', 'broadcast', 'sigmoid', False, 'gaussian'),
    (31, 10, 5, 130, 'intended', 'aligned', 'relu', True, 'identity'),
    (31, 10, 1, 64, 'reference', 'broadcast', 'relu', False, 'relu'),
    (31, 16, 4, 1, 'reference', 'aligned', 'tanh', True, 'sigmoid'),
    (31, 16, 9, 65, 'intended', 'broadcast', 'identity', False, 'tanh'),
]


def _head_problem(D, K, ntn_mode, loss_mode, inneract, bias, final):
    flags = dict(final_act='sim_kernel', sim_kernel='gaussian') if final == 'gaussian' else \
        dict(final_act=final)
    ov = ntn_stack(D, K, inneract, bias, dropout=0.0, ntn_mode=ntn_mode, loss_mode=loss_mode,
                   **flags)
    prob = sized_problem([1, 2, min(D, 10)], ov, n_max=D, seed=100 + D + K)
    # U >= 0 with mean |U| / K: the score stays O(1), so tanh / sigmoid / gaussian final
    # activations are not saturated (where fp32's 1 - ŷ² has no significant bit left and the
    # float64 gradient is ~1e-11) and a relu final activation sees positive scores
    o, _ = _offsets(prob)[0][(len(prob.layers) - 1, 'weights_U')]
    prob.params[o:o + K] = np.abs(prob.params[o:o + K]) / K
    return prob


def _autograd_head(prob, eq, edb, labels, ystats, add_label):
    """The NTN head (layers.py:282-310), final activation and loss (model_mse.py:145-151)
    restated in float64 torch on the CPU; returns scores, loss, the smallest |m_k| and |s|,
    and the gradients of the embeddings and of every head variable."""
    import torch
    f = prob.flags
    offs, _ = _offsets(prob)
    hi = len(prob.layers) - 1
    L = prob.layers[hi]
    D, K = L['input_dim'], L['feature_map_dim']
    flat = torch.from_numpy(prob.params.astype(np.float64))

    def var(name):
        o, shape = offs[(hi, name)]
        return flat[o:o + int(np.prod(shape))].reshape(shape).clone().requires_grad_(True)
    W, V, U = var('weights_W'), var('weights_V'), var('weights_U')
    b = var('bias') if L['bias'] else None
    e1 = torch.from_numpy(eq.astype(np.float64)).requires_grad_(True)
    e2 = torch.from_numpy(edb.astype(np.float64)).requires_grad_(True)
    mk = torch.einsum('ia,abk,jb->ijk', e1, W, e2) + (e1 @ V[:, :D].T)[:, None, :] + \
        (e2 @ V[:, D:].T)[None, :, :]
    if b is not None:
        mk = mk + b
    act = {'relu': torch.relu, 'sigmoid': torch.sigmoid, 'tanh': torch.tanh,
           'identity': lambda x: x}[L['inneract']]
    r = act(mk)
    u = U[:, 0]
    s = u.sum() * r.sum(-1) if f.ntn_mode == 'reference' else r @ u
    if f.final_act == 'sim_kernel':
        yhat = torch.exp(-f.yeta * s * s)
    else:
        yhat = {'relu': torch.relu, 'sigmoid': torch.sigmoid, 'tanh': torch.tanh,
                'identity': lambda x: x}[f.final_act](s)
    y = torch.from_numpy(labels.astype(np.float64))
    if f.loss_mode == 'broadcast':
        loss = 0.5 * ((yhat - float(ystats[0])) ** 2).sum() + (float(ystats[1]) if add_label else 0.0)
    else:
        loss = 0.5 * ((yhat - y) ** 2).sum() / y.numel()
    loss.backward()
    grads = {'weights_W': W.grad, 'weights_V': V.grad, 'weights_U': U.grad}
    if b is not None:
        grads['bias'] = b.grad
    return (s.detach().numpy(), float(loss.item()), float(mk.detach().abs().min()),
            float(s.detach().abs().min()), e1.grad.numpy(), e2.grad.numpy(),
            {k: v.numpy() for k, v in grads.items()})


def _run_grid(model, eq, edb, labels, ystats, add_label, pad_lab=5, pad_s=3):
    """sg_score_grid_fwd_bwd with ld_labels = n + pad_lab, ld_s = n + pad_s, sentinel-filled
    outputs; returns torch tensors (s [m][n + pad_s], g_q, g_db, grad, loss)."""
    import torch
    from graphembedding_amd import _lib
    dev = model.params.device
    m, n = eq.shape[0], edb.shape[0]
    lab = torch.full((m, n + pad_lab), 99.0, dtype=torch.float32, device=dev)
    lab[:, :n] = torch.from_numpy(labels).to(dev)
    s = torch.full((m, n + pad_s), SENTINEL, dtype=torch.float32, device=dev)
    gq = torch.full((m, eq.shape[1]), SENTINEL, dtype=torch.float32, device=dev)
    gdb = torch.full((n, eq.shape[1]), SENTINEL, dtype=torch.float32, device=dev)
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.score_grid_bwd_workspace_bytes(model.sg, m, n) // 4 + 1,
                     dtype=torch.float32, device=dev)
    ys = torch.from_numpy(ystats).to(dev)
    _lib.score_grid_fwd_bwd(model.sg, torch.from_numpy(eq).to(dev), torch.from_numpy(edb).to(dev),
                            m, n, model.params, lab, n + pad_lab, m * n, ys, add_label, s,
                            n + pad_s, gq, gdb, grad, loss, ws)
    torch.cuda.synchronize()
    return s, gq, gdb, grad, loss


def _draw(D, m, n, seed):
    rng = np.random.default_rng(seed)
    eq = rng.uniform(-0.7, 0.7, size=(m, D)).astype(np.float32)
    edb = rng.uniform(-0.7, 0.7, size=(n, D)).astype(np.float32)
    labels = rng.uniform(0.05, 1.0, size=(m, n)).astype(np.float32)
    y = labels.astype(np.float64)
    ystats = np.array([y.mean(), 0.5 * ((y - y.mean()) ** 2).sum()], np.float32)
    return eq, edb, labels, ystats


@pytest.mark.parametrize('case', GRID_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_grid_adjoint_matches_autograd(gpu, case):
    D, K, m, n, ntn_mode, loss_mode, inneract, bias, final = case
    prob = _head_problem(D, K, ntn_mode, loss_mode, inneract, bias, final)
    model = gpu_model(prob, gpu)
    add_label = (m + n) % 2 == 0
    # inputs whose float64 pre-activations keep clear of the relu kinks: a tie there is a
    # matter of rounding, not of parity
    for seed in range(20):
        eq, edb, labels, ystats = _draw(D, m, n, 1000 * D + 10 * K + seed)
        s_ref, l_ref, min_m, min_s, gq_ref, gdb_ref, head_ref = _autograd_head(
            prob, eq, edb, labels, ystats, add_label)
        if (inneract != 'relu' or min_m > 1e-6) and (final != 'relu' or min_s > 1e-6) and \
                np.abs(gq_ref).max() > 1e-6:
            break
    # the reference gradient is far above fp32 noise: the check below means something
    assert np.abs(gq_ref).max() > 1e-6 and np.abs(gdb_ref).max() > 1e-6
    if inneract == 'relu':
        assert min_m > 1e-6, min_m
    if final == 'relu':
        assert min_s > 1e-6, min_s
    s, gq, gdb, grad, loss = _run_grid(model, eq, edb, labels, ystats, add_label)
    s = s.cpu().numpy()
    assert np.all(s[:, n:] == SENTINEL), 'columns j >= n of s_out were written'
    print('max |s - ref|', float(np.abs(s[:, :n] - s_ref).max()), 'loss', float(loss.item()), l_ref)
    np.testing.assert_allclose(s[:, :n], s_ref, rtol=TOL, atol=TOL)
    assert abs(float(loss.item()) - l_ref) <= TOL * max(1.0, abs(l_ref)), (float(loss.item()), l_ref)
    _block_close(gq.cpu().numpy(), gq_ref, 'g_emb_q')
    _block_close(gdb.cpu().numpy(), gdb_ref, 'g_emb_db')
    offs, total = _offsets(prob)
    hi = len(prob.layers) - 1
    g = grad.cpu().numpy()
    head0 = offs[(hi, 'weights_W')][0]
    assert np.all(g[:head0] == SENTINEL), 'the node-layer range of grad_out was written'
    covered = head0
    for name, want in head_ref.items():
        o, shape = offs[(hi, name)]
        _block_close(g[o:o + want.size].reshape(shape), want, name)
        covered += want.size
    assert covered == total == model.n_params


# ---- 2. determinism ---------------------------------------------------------------------
def test_grid_is_bitwise_deterministic(gpu):
    """Four column blocks and ten query chunks: every cross-workgroup sum is exercised."""
    import torch
    prob = _head_problem(10, 10, 'reference', 'broadcast', 'relu', True, 'gaussian')
    model = gpu_model(prob, gpu)
    eq, edb, labels, ystats = _draw(10, 37, 200, 5)
    a = _run_grid(model, eq, edb, labels, ystats, True)
    b = _run_grid(model, eq, edb, labels, ystats, True)
    head0 = _offsets(prob)[0][(len(prob.layers) - 1, 'weights_W')][0]
    for x, y, what in zip(a, b, ('s', 'g_emb_q', 'g_emb_db', 'grad', 'loss')):
        assert torch.equal(x, y), what
    assert float(a[3][head0:].abs().max().item()) > 0


# ---- 3. sg_embed_bwd against the oracle's _node_backward --------------------------------
EMBED_STACKS = {   # name: (flag overrides, n_max = Padding dim)
    'default': ({}, 10),
    'average': (AVERAGE_STACK, 10),
    'attention': (ATTENTION_STACK, 10),
    'dense_after_pad': (DENSE_AFTER_PAD, 10),
    'pad30_nmax32': ({}, 30),
}


def _embed_problem(name):
    ov, pd = EMBED_STACKS[name]
    rng = np.random.default_rng(3)
    counts = [1, 8, 9, pd] + [int(x) for x in rng.integers(1, pd + 1, size=8)]
    return sized_problem(counts, dict(ov, dropout=0.0), n_max=pd, seed=11)


def _oracle_embed_bwd(prob, idx, g_emb):
    """Σ_c _node_backward of graph idx[c] seeded with g_emb[c] (entries with idx < 0 are
    skipped): the flat gradient, head range zero."""
    spec = prob.oracle_spec()
    P = O.unflatten(spec, prob.params.astype(np.float64))
    G = {k: np.zeros_like(v) for k, v in P.items()}
    gs = oracle_graphs(prob)
    for c, gi in enumerate(idx):
        if gi < 0:
            continue
        x, caches = O._node_forward(spec, P, gs[gi], 0, 0, 0)
        O._node_backward(spec, P, G, gs[gi], caches,
                         np.asarray(g_emb[c], np.float64).reshape(np.shape(x)))
    return O.flatten(spec, G)


def _run_embed_bwd(model, dev_store, idx, g_emb):
    import torch
    from graphembedding_amd import _lib
    dev = model.params.device
    count = len(idx)
    idx_t = torch.as_tensor(np.asarray(idx), dtype=torch.int32, device=dev)
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.embed_bwd_workspace_bytes(model.sg, count) // 4 + 1,
                     dtype=torch.float32, device=dev)
    _lib.embed_bwd(model.sg, dev_store, model.n_max, idx_t, count, model.params,
                   torch.from_numpy(g_emb).to(dev), grad, ws, status)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), int(status.item())


def _check_node_range(prob, got, want):
    """Node-layer variables per variable at TOL; the head's range still holds the sentinel."""
    offs, total = _offsets(prob)
    hi = len(prob.layers) - 1
    head0 = min(o for (li, _), (o, _) in offs.items() if li == hi) if \
        prob.layers[hi]['kind'] == 'NTN' else total
    assert np.all(got[head0:] == SENTINEL), 'the head range of grad_out was written'
    for (li, name), (o, shape) in offs.items():
        if li != hi:
            n = int(np.prod(shape))
            _block_close(got[o:o + n], want[o:o + n], '{}.{}'.format(li, name))


@pytest.mark.parametrize('name', list(EMBED_STACKS))
def test_embed_bwd_matches_oracle(gpu, name):
    from graphembedding_amd.packer import GraphStore
    prob = _embed_problem(name)
    model = gpu_model(prob, gpu)
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    G, E = len(store), model.embed_dim
    rng = np.random.default_rng(17)
    for count in (7, 12):   # an odd tail; permuted with repeats either way
        idx = rng.integers(0, G, size=count)
        idx[:4] = rng.permutation(4)           # node counts 1, 8, 9 and the Padding dim
        idx[-1] = idx[0]                       # a repeat
        g_emb = rng.standard_normal((count, E)).astype(np.float32)
        got, st = _run_embed_bwd(model, store.to_device(gpu), idx, g_emb)
        assert st == 0
        _check_node_range(prob, got, _oracle_embed_bwd(prob, idx, g_emb))


def test_embed_bwd_status_and_zero_contribution(gpu):
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import GraphStore
    prob = _embed_problem('default')
    model = gpu_model(prob, gpu)
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    E = model.embed_dim
    rng = np.random.default_rng(23)
    g_emb = rng.standard_normal((5, E)).astype(np.float32)
    dev = store.to_device(gpu)
    # a bad id next to a good graph, and a wavefront whose two graphs are both bad
    for idx in ([0, 10_000, 2, 3, 4], [10_000, -5, 1, 2, 3]):
        got, st = _run_embed_bwd(model, dev, idx, g_emb)
        assert st == _lib.SG_ERR_ARG
        kept = [i if 0 <= i < len(store) else -1 for i in idx]
        _check_node_range(prob, got, _oracle_embed_bwd(prob, kept, g_emb))
    # a node count of 0: SG_ERR_SHAPE, nothing from that entry
    adj, types, n = dev
    n0 = n.clone()
    n0[2] = 0
    got, st = _run_embed_bwd(model, (adj, types, n0), [0, 1, 2, 3, 4], g_emb)
    assert st == _lib.SG_ERR_SHAPE
    _check_node_range(prob, got, _oracle_embed_bwd(prob, [0, 1, -1, 3, 4], g_emb))


# ---- 4. end to end against the pairwise path --------------------------------------------
def _e2e_problem(stack, n_graphs, seed):
    rng = np.random.default_rng(seed)
    counts = [1, 10] + [int(x) for x in rng.integers(2, 11, size=n_graphs - 2)]
    return sized_problem(counts, dict(stack, dropout=0.0), n_max=10, seed=seed)


def _pairwise_batch(model, store, q, db, labels):
    import torch
    pairs = np.stack([np.repeat(q, len(db)), np.tile(db, len(q))], axis=1).astype(np.int32)
    pi = torch.from_numpy(pairs).to(model.params.device)
    lab = torch.from_numpy(labels.reshape(-1).copy()).to(model.params.device)
    return model.batch_from_store(store, len(pairs), lab, pair_idx=pi), pairs


E2E = {'9x70': (79, np.arange(70, 79), np.arange(70)), '12x12': (12, None, None)}


@pytest.mark.parametrize('shape', list(E2E))
@pytest.mark.parametrize('stack', ['default', 'average'])
def test_grid_fwd_bwd_matches_pairwise_and_oracle(gpu, stack, shape):
    import torch
    from graphembedding_amd.allpairs import AllPairsGrid, GraphSet
    from graphembedding_amd.packer import GraphStore
    n_graphs, q, db = E2E[shape]
    prob = _e2e_problem(EMBED_STACKS[stack][0], n_graphs, 31 + n_graphs)
    model = gpu_model(prob, gpu)
    assert model.kernel_path == 1 and model.sg.keep_prob == 1.0
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    qa = np.arange(n_graphs) if q is None else q
    da = np.arange(n_graphs) if db is None else db
    labels = np.random.default_rng(2).uniform(0.05, 1.0, size=(len(qa), len(da))).astype(np.float32)
    if q is None:   # the all-pairs grid through AllPairsGrid
        gs = GraphSet(graphs=prob.graphs, mgs=prob.mgs, d_in=prob.d_in, n_max=model.n_max,
                      store=store, ged=None)
        grid = AllPairsGrid(gs, labels, gpu)
        grid.fwd_bwd(model)
        grid.problem(model).check()
    else:
        model.grid_fwd_bwd(store, labels, q, db).check()
    g_grid = model.grad.cpu().numpy().copy()
    l_grid = float(model.loss_buf[0].item())
    # the pairwise fused path over the same pairs, same parameters
    batch, pairs = _pairwise_batch(model, store, qa, da, labels)
    model.fwd_bwd(batch, seed=0)
    g_pair = model.grad.cpu().numpy().copy()
    l_pair = float(model.loss_buf[0].item())
    gs_o = oracle_graphs(prob)
    ref = O.fwd_bwd(prob.oracle_spec(), prob.params.astype(np.float64),
                    [gs_o[i] for i in pairs[:, 0]], [gs_o[j] for j in pairs[:, 1]],
                    labels.reshape(-1).astype(np.float64), 0)
    print('loss grid', l_grid, 'pairwise', l_pair, 'oracle', ref.loss_mse)
    assert abs(l_grid - ref.loss_mse) <= TOL * max(1.0, abs(ref.loss_mse))
    assert abs(l_grid - l_pair) <= TOL * max(1.0, abs(l_pair))
    print(check_grad_per_var(g_grid, ref.grad_mse, prob.layers, prob.d_in, TOL, 'grid vs oracle'))
    print(check_grad_per_var(g_grid, g_pair, prob.layers, prob.d_in, TOL, 'grid vs pairwise'))
    # scores on request
    s = torch.empty((len(qa), len(da)), dtype=torch.float32, device=gpu)
    model.grid_fwd_bwd(store, labels, q, db, s_out=s)
    np.testing.assert_allclose(s.cpu().numpy().reshape(-1), ref.s, rtol=TOL, atol=TOL)


@pytest.mark.parametrize('stack', ['default', 'average'])
def test_three_grid_train_steps_match_pairwise_adam(gpu, stack):
    from graphembedding_amd.packer import GraphStore
    n_graphs, q, db = E2E['9x70']
    prob = _e2e_problem(EMBED_STACKS[stack][0], n_graphs, 31 + n_graphs)
    a, b = gpu_model(prob, gpu), gpu_model(prob, gpu)
    store = GraphStore(prob.mgs, a.n_max, prob.d_in)
    labels = np.random.default_rng(2).uniform(0.05, 1.0, size=(len(q), len(db))).astype(np.float32)
    gp = a.grid_problem(store, labels, q, db)
    batch, _ = _pairwise_batch(b, store, q, db, labels)
    for step in range(3):
        la = a.grid_train_step(gp)
        lb = b.train_step(batch, seed=0)
        assert abs(la - lb) <= TOL * max(1.0, abs(lb)), (step, la, lb)
    gp.check()
    assert a.step_count == b.step_count == 3
    err = float((a.params - b.params).abs().max().item())
    moved = float((a.params - a.torch.from_numpy(prob.params).to(gpu)).abs().max().item())
    print('max |param diff| after 3 steps', err, 'moved', moved)
    assert moved > 1e-3
    assert err <= 1e-4, err


# ---- 5. refusal -------------------------------------------------------------------------
def test_grid_training_refuses_dropout(gpu):
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import GraphStore
    prob = _e2e_problem({}, 12, 43)
    model = gpu_model(prob, gpu, dropout=0.1)
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    labels = np.full((12, 12), 0.5, np.float32)
    before = model.grad_loss.clone()
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.grid_fwd_bwd(store, labels)
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.grid_train_step(store, labels)
    assert model.torch.equal(before, model.grad_loss) and model.step_count == 0
    # the C ABI refuses on its own, whatever the Python layer checked
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        _lib.score_grid_bwd_workspace_bytes(model.sg, 12, 12)
