"""Embed-once training of Dot-head models on the GPU (include/siamese_dot_embed.h): the grid's
forward, loss and adjoint against a float64 numpy restatement, its bitwise determinism and
its scores against sg_dot_score_grid; grid_fwd_bwd / grid_train_step end to end against the
pair path and the oracle; graph-keyed dropout through AllPairsGrid.
Bars are the project's: scores and loss within 1e-4 (rtol = atol, test_gpu_parity.TOL), every
gradient block within 1e-4 of its own largest component (test_gpu_embed_train._block_close,
_fixtures.check_grad_per_var), parameters after Adam steps at the zoo's atol 2e-5."""
import numpy as np
import pytest

import _stack_zoo as Z
from _embed_fixtures import gpu_model, oracle_graphs
from _fixtures import check_grad_per_var
from oracle import siamese_oracle as O
from test_dot_embed_abi import dot_model
from test_gpu_dot_grid import pair_batch
from test_gpu_embed_train import _block_close

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -7.25
YETA = 0.6

# E -> (Padding rows, width)
SHAPES = {1: (1, 1), 6: (2, 3), 17: (1, 17), 160: (10, 16)}
CALL_CASES = [(1, 1, 1), (5, 65, 6), (33, 130, 17), (64, 64, 160)]
FINALS = ('gaussian', 'identity', 'relu', 'sigmoid', 'tanh')


def _final_flags(final):
    return dict(final_act='sim_kernel', sim_kernel='gaussian', yeta=YETA) if final == 'gaussian' \
        else dict(final_act=final)


def _numpy_ref(eq, edb, labels, ystats, final, loss_mode, add_label):
    """Scores, loss, g_emb_q, g_emb_db of the Dot head + final activation + loss in float64."""
    e1, e2 = eq.astype(np.float64), edb.astype(np.float64)
    s = e1 @ e2.T
    if final == 'gaussian':
        yhat = np.exp(-YETA * s * s)
        dy = -2.0 * YETA * s * yhat
    elif final == 'identity':
        yhat, dy = s, np.ones_like(s)
    elif final == 'relu':
        yhat, dy = np.maximum(s, 0.0), (s > 0).astype(np.float64)
    elif final == 'sigmoid':
        yhat = 1.0 / (1.0 + np.exp(-s))
        dy = yhat * (1.0 - yhat)
    else:
        yhat = np.tanh(s)
        dy = 1.0 - yhat * yhat
    if loss_mode == 'broadcast':
        gy = yhat - float(ystats[0])
        loss = 0.5 * (gy ** 2).sum() + (float(ystats[1]) if add_label else 0.0)
    else:
        d = yhat - labels.astype(np.float64)
        gy = d / d.size
        loss = 0.5 * (d ** 2).sum() / d.size
    gs = gy * dy
    return s, loss, gs @ e2, gs.T @ e1, float(np.abs(s).min())


def _run(gpu, sg, eq, edb, labels, ystats, add_label, pad=3):
    """sg_dot_score_grid_fwd_bwd with strided inputs, labels and scores, and two sentinel rows
    after g_emb_q / g_emb_db; returns (s [m][n + pad], gq [m + 2][E], gdb [n + 2][E], loss)."""
    import torch
    from graphembedding_amd import _lib
    m, n, E = eq.shape[0], edb.shape[0], eq.shape[1]
    bq = torch.full((m, E + 2), float('nan'), dtype=torch.float32, device=gpu)
    bdb = torch.full((n, E + 1), float('nan'), dtype=torch.float32, device=gpu)
    bq[:, :E] = torch.from_numpy(eq).to(gpu)
    bdb[:, :E] = torch.from_numpy(edb).to(gpu)
    lab = torch.full((m, n + 5), 99.0, dtype=torch.float32, device=gpu)
    lab[:, :n] = torch.from_numpy(labels).to(gpu)
    s = torch.full((m, n + pad), SENTINEL, dtype=torch.float32, device=gpu)
    gq = torch.full((m + 2, E), SENTINEL, dtype=torch.float32, device=gpu)
    gdb = torch.full((n + 2, E), SENTINEL, dtype=torch.float32, device=gpu)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=gpu)
    ws = torch.empty(_lib.dot_score_grid_bwd_workspace_bytes(sg, m, n) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    _lib.dot_score_grid_fwd_bwd(sg, bq, E + 2, bdb, E + 1, m, n, lab, n + 5, m * n,
                                torch.from_numpy(ystats).to(gpu), add_label, s, n + pad, gq, gdb,
                                loss, ws)
    plain = torch.empty((m, n), dtype=torch.float32, device=gpu)
    _lib.dot_score_grid(sg, bq, E + 2, bdb, E + 1, m, n, False, plain, n)
    torch.cuda.synchronize()
    return s, gq, gdb, loss, plain


def _draw(E, m, n, seed, final):
    rng = np.random.default_rng(seed)
    scale = 0.9 / np.sqrt(E)          # |s| = O(1): no final activation is saturated
    eq = (scale * rng.uniform(0.5, 1.5, (m, E)) * rng.choice([-1.0, 1.0], (m, E))).astype(np.float32)
    edb = (scale * rng.uniform(0.5, 1.5, (n, E)) * rng.choice([-1.0, 1.0], (n, E))).astype(np.float32)
    if m * n == 1:                    # the only score is positive: a relu final has a gradient
        eq, edb = np.abs(eq), np.abs(edb)
    labels = rng.uniform(0.05, 1.0, size=(m, n)).astype(np.float32)
    y = labels.astype(np.float64)
    ystats = np.array([y.mean(), 0.5 * ((y - y.mean()) ** 2).sum()], np.float32)
    return eq, edb, labels, ystats


@pytest.mark.parametrize('final', FINALS)
@pytest.mark.parametrize('loss_mode', ['broadcast', 'aligned'])
@pytest.mark.parametrize('case', CALL_CASES, ids=lambda c: 'x'.join(str(x) for x in c))
def test_dot_grid_call_matches_numpy(gpu, case, loss_mode, final):
    import torch
    m, n, E = case
    sg = dot_model(*SHAPES[E], loss_mode=loss_mode, **_final_flags(final))
    for add_label in (True, False):
        eq, edb, labels, ystats = _draw(E, m, n, 100 * E + m + (7 if add_label else 0), final)
        s_ref, l_ref, gq_ref, gdb_ref, min_s = _numpy_ref(eq, edb, labels, ystats, final,
                                                           loss_mode, add_label)
        if final == 'relu':   # scores clear of the kink: a tie there is a matter of rounding
            assert min_s > 1e-6, min_s
        s, gq, gdb, loss, plain = _run(gpu, sg, eq, edb, labels, ystats, add_label)
        assert torch.equal(s[:, :n], plain), 'scores differ from sg_dot_score_grid'
        assert bool((s[:, n:] == SENTINEL).all()), 'columns j >= n of s_out were written'
        assert bool((gq[m:] == SENTINEL).all()) and bool((gdb[n:] == SENTINEL).all())
        np.testing.assert_allclose(s[:, :n].cpu().numpy(), s_ref, rtol=TOL, atol=TOL)
        got_l = float(loss.item())
        print('loss', got_l, l_ref)
        assert abs(got_l - l_ref) <= TOL * max(1.0, abs(l_ref)), (got_l, l_ref)
        assert np.abs(gq_ref).max() > 1e-7 and np.abs(gdb_ref).max() > 1e-7
        _block_close(gq[:m].cpu().numpy(), gq_ref, 'g_emb_q')
        _block_close(gdb[:n].cpu().numpy(), gdb_ref, 'g_emb_db')
        again = _run(gpu, sg, eq, edb, labels, ystats, add_label)
        for a, b, what in zip((s, gq, gdb, loss), again, ('s', 'g_emb_q', 'g_emb_db', 'loss')):
            assert torch.equal(a, b), what


def test_dot_grid_call_sums_partials_deterministically(gpu):
    """m and n above the 512-row chunk of the adjoint's partial products and many 64 x 64
    tiles: every cross-workgroup sum runs, twice, to the same bits."""
    import torch
    m, n, E = 600, 530, 6
    sg = dot_model(*SHAPES[E])
    eq, edb, labels, ystats = _draw(E, m, n, 5, 'gaussian')
    s_ref, l_ref, gq_ref, gdb_ref, _ = _numpy_ref(eq, edb, labels, ystats, 'gaussian',
                                                  'broadcast', True)
    a = _run(gpu, sg, eq, edb, labels, ystats, True)
    b = _run(gpu, sg, eq, edb, labels, ystats, True)
    for x, y, what in zip(a, b, ('s', 'g_emb_q', 'g_emb_db', 'loss', 'plain')):
        assert torch.equal(x, y), what
    assert abs(float(a[3].item()) - l_ref) <= TOL * max(1.0, abs(l_ref))
    _block_close(a[1][:m].cpu().numpy(), gq_ref, 'g_emb_q')
    _block_close(a[2][:n].cpu().numpy(), gdb_ref, 'g_emb_db')


# ---- end to end against the pair path and the oracle -------------------------------------
def _pairwise_batch(model, store, q, db, labels):
    pairs = np.stack([np.repeat(q, len(db)), np.tile(db, len(q))], axis=1).astype(np.int32)
    return pair_batch(model, store, pairs, labels), pairs


E2E_NAMES = ('dot_average_tanh_aligned', 'nmax7')       # one Average, one Padding
Q_IDX = np.array([8, 0, 3, 8])                          # 9 graphs, repeats in both roles
DB_IDX = np.array([1, 2, 0, 4, 5, 6, 7, 2, 3])


def _e2e(name, gpu):
    from graphembedding_amd.packer import GraphStore
    prob = Z.zoo_problem(name, 0.0)
    model = gpu_model(prob, gpu)
    assert model.is_dot
    mgs = prob.mgs[:9]
    store = GraphStore(mgs, model.n_max, prob.d_in)
    labels = np.random.default_rng(2).uniform(0.05, 1.0, size=(len(Q_IDX), len(DB_IDX))).astype(
        np.float32)
    return prob, model, store, labels


@pytest.mark.parametrize('name', E2E_NAMES)
def test_dot_grid_fwd_bwd_matches_pairwise_and_oracle(gpu, name):
    import torch
    prob, model, store, labels = _e2e(name, gpu)
    s = torch.empty(labels.shape, dtype=torch.float32, device=gpu)
    model.grid_fwd_bwd(store, labels, Q_IDX, DB_IDX, s_out=s).check()
    g_grid = model.grad.cpu().numpy().copy()
    l_grid = float(model.loss_buf[0].item())
    batch, pairs = _pairwise_batch(model, store, Q_IDX, DB_IDX, labels)
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
    np.testing.assert_allclose(s.cpu().numpy().reshape(-1), ref.s, rtol=TOL, atol=TOL)


@pytest.mark.parametrize('name', E2E_NAMES)
def test_three_dot_grid_train_steps_match_pairwise_adam(gpu, name):
    prob, a, store, labels = _e2e(name, gpu)
    b = gpu_model(prob, gpu)
    gp = a.grid_problem(store, labels, Q_IDX, DB_IDX)
    batch, _ = _pairwise_batch(b, store, Q_IDX, DB_IDX, labels)
    for step in range(3):
        la = a.grid_train_step(gp)
        lb = b.train_step(batch, seed=0)
        assert abs(la - lb) <= TOL * max(1.0, abs(lb)), (step, la, lb)
    gp.check()
    assert a.step_count == b.step_count == 3
    moved = float((a.params - a.torch.from_numpy(prob.params).to(gpu)).abs().max().item())
    assert moved > 1e-3
    np.testing.assert_allclose(a.params.cpu().numpy(), b.params.cpu().numpy(), rtol=0, atol=2e-5)


# ---- graph-keyed dropout through AllPairsGrid --------------------------------------------
def _grid_set(prob, model):
    from graphembedding_amd.allpairs import GraphSet
    from graphembedding_amd.packer import GraphStore
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    return GraphSet(graphs=prob.graphs, mgs=prob.mgs, d_in=prob.d_in, n_max=model.n_max,
                    store=store, ged=None)


def test_all_pairs_grid_graph_dropout_on_a_dot_model(gpu):
    from graphembedding_amd.allpairs import AllPairsGrid
    name = 'dot_average_tanh_broadcast'
    prob = Z.zoo_problem(name)                     # the entry's own dropout: > 0
    assert prob.flags.dropout > 0
    model = gpu_model(prob, gpu)
    G = len(prob.mgs)
    labels = np.random.default_rng(3).uniform(0.05, 1.0, size=(G, G)).astype(np.float32)
    grid = AllPairsGrid(_grid_set(prob, model), labels, gpu, dropout='graph')
    losses = [grid.train_step(model) for _ in range(3)]
    grid.problem(model).check()
    print('losses', losses)
    assert all(np.isfinite(x) for x in losses)
    assert len(set(losses)) == 3                   # new masks and new parameters every step


def test_graph_dropout_equals_none_at_dropout_zero(gpu):
    import torch
    from graphembedding_amd.allpairs import AllPairsGrid
    name = 'dot_attention_relu_aligned'
    prob = Z.zoo_problem(name, 0.0)
    G = len(prob.mgs)
    labels = np.random.default_rng(4).uniform(0.05, 1.0, size=(G, G)).astype(np.float32)
    out = {}
    for dropout in (None, 'graph'):
        model = gpu_model(prob, gpu)
        grid = AllPairsGrid(_grid_set(prob, model), labels, gpu, dropout=dropout)
        s = torch.empty((G, G), dtype=torch.float32, device=gpu)
        model.grid_fwd_bwd(grid.problem(model), s_out=s)
        out[dropout] = (float(model.loss_buf[0].item()), s.clone(), model.grad.cpu().numpy().copy())
    assert out[None][0] == out['graph'][0]
    assert torch.equal(out[None][1], out['graph'][1])
    # the node backward sums with LDS atomics: the gradient is held to TOL only
    print(check_grad_per_var(out['graph'][2], out[None][2], prob.layers, prob.d_in, TOL,
                             'graph vs none'))
