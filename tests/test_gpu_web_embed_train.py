"""Embed-once training for graph-store (Web) models on the GPU
(include/siamese_web_embed_train.h): the large-D NTN grid's forward, loss and adjoint against
float64 torch autograd, its contract (bitwise scores, determinism, strides, untouched
padding), the CSR node-stack backward against the oracle's _node_backward, and
web_grid_fwd_bwd / web_grid_train_step end to end against the pairwise path (sg_web_fwd_bwd).
Bars are the project's: scores and loss within 1e-4·(1 + |value|), every gradient block within
1e-4 of its own largest component (_fixtures.check_grad_per_var), three free-running Adam steps
within the 1e-4 of test_gpu_trajectory."""
import os

import numpy as np
import pytest

from _embed_fixtures import gpu_model, ntn_stack, oracle_graphs, signed_embeddings, sized_problem
from _fixtures import check_grad_per_var
from oracle import siamese_oracle as O
from test_gpu_embed_train import _autograd_head, _block_close, _offsets
from test_gpu_web_embed import _alive, _case, _csr

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -7.25
QC_ENV = 'SG_WEB_TRAIN_QC'   # at most this many queries per chunk (read per call)


# ---- 1. the grid's adjoint against autograd ---------------------------------------------
# (D, K, m, n, ntn_mode, loss_mode, bias, final, qc): the issue's shapes, the options spread
# over them; the last case runs chunks of 4 queries (m = 9: 4 + 4 + 1) over three 64-row
# blocks.  D covers every A-operand instantiation (17, 33, 65, 97, 129 k-steps), D % 4 in
# {0, 1, 2}, a table of one tile (K = 1) and the full tile (K = 16).
GRID_CASES = [
    (33, 10, 5, 65, 'reference', 'broadcast', True, 'gaussian', 0),
    (50, 1, 4, 63, 'intended', 'aligned', False, 'sigmoid', 0),
    (64, 16, 9, 130, 'reference', 'aligned', True, 'tanh', 0),
    (68, 10, 1, 64, 'intended', 'broadcast', False, 'relu', 0),
    (132, 10, 33, 1, 'reference', 'aligned', True, 'identity', 0),
    (260, 16, 5, 65, 'intended', 'broadcast', True, 'gaussian', 0),
    (388, 10, 4, 64, 'reference', 'broadcast', False, 'tanh', 0),
    (512, 16, 5, 70, 'intended', 'aligned', True, 'sigmoid', 0),
    (64, 10, 9, 130, 'intended', 'aligned', True, 'gaussian', 4),
]


def _head_problem(D, K, ntn_mode, loss_mode, bias, final):
    flags = dict(final_act='sim_kernel', sim_kernel='gaussian') if final == 'gaussian' else \
        dict(final_act=final)
    ov = ntn_stack(D, K, 'relu', bias, dropout=0.0, ntn_mode=ntn_mode, loss_mode=loss_mode,
                   **flags)
    prob = sized_problem([1, D], ov, n_max=D, seed=100 + D + K, n_types=60 if D > 400 else 29)
    o, _ = _offsets(prob)[0][(len(prob.layers) - 1, 'weights_U')]
    prob.params[o:o + K] = np.abs(prob.params[o:o + K]) / K
    return prob, o


def _draw(D, m, n, seed):
    eq = signed_embeddings(m, D, seed)
    edb = signed_embeddings(n, D, seed + 1)
    rng = np.random.default_rng(seed)
    labels = rng.uniform(0.05, 1.0, size=(m, n)).astype(np.float32)
    y = labels.astype(np.float64)
    return eq, edb, labels, np.array([y.mean(), 0.5 * ((y - y.mean()) ** 2).sum()], np.float32)


def _unsaturated_case(case):
    """The case's problem, inputs and float64 reference, chosen on the CPU.
    Dense signed embeddings give m_k of magnitude ~ D · |W|, so with U = |U| / K alone the
    score is far in the tail of tanh / sigmoid / gaussian, where fp32 has no significant bit
    of 1 - ŷ² left.  The score is linear in U and m_k does not depend on it, so U is divided
    by the power of two that brings max |s| of the float64 reference to at most 1.  The seed
    is the first for which no relu sits within 1e-3 of its kink."""
    D, K, m, n, ntn_mode, loss_mode, bias, final, _ = case
    prob, oU = _head_problem(D, K, ntn_mode, loss_mode, bias, final)
    add_label = (m + n) % 2 == 0
    u0 = prob.params[oU:oU + K].copy()
    for seed in range(60):
        eq, edb, labels, ystats = _draw(D, m, n, 7000 + 100 * D + seed)
        prob.params[oU:oU + K] = u0
        ref = _autograd_head(prob, eq, edb, labels, ystats, add_label)
        if ref[2] <= 1e-3:
            continue
        smax = float(np.abs(ref[0]).max())
        if smax > 1.0:
            prob.params[oU:oU + K] = u0 * np.float32(2.0 ** -int(np.ceil(np.log2(smax))))
            ref = _autograd_head(prob, eq, edb, labels, ystats, add_label)
        return prob, eq, edb, labels, ystats, add_label, ref
    raise AssertionError('no seed keeps every m_k clear of the relu kink')


def _run_grid(model, eq, edb, labels, ystats, add_label, ld_e=None, pad_lab=5, pad_s=3,
              pad_g=6, want_s=True, want_loss=True):
    """sg_web_score_grid_fwd_bwd with embeddings of row stride ld_e (default D), padded and
    sentinel-filled outputs; returns torch tensors (s, g_q, g_db, grad, loss)."""
    import torch
    from graphembedding_amd import _lib
    dev = model.params.device
    (m, D), n = eq.shape, edb.shape[0]
    ld_e = ld_e or D

    def rows(e):
        t = torch.full((e.shape[0], ld_e), 3.5, dtype=torch.float32, device=dev)
        t[:, :D] = torch.from_numpy(e).to(dev)
        return t
    lab = torch.full((m, n + pad_lab), 99.0, dtype=torch.float32, device=dev)
    lab[:, :n] = torch.from_numpy(labels).to(dev)
    s = torch.full((m, n + pad_s), SENTINEL, dtype=torch.float32, device=dev)
    gq = torch.full((m, D + pad_g), SENTINEL, dtype=torch.float32, device=dev)
    gdb = torch.full((n, D + pad_g + 1), SENTINEL, dtype=torch.float32, device=dev)
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.web_score_grid_bwd_workspace_bytes(model.sg, m, n) // 4 + 1,
                     dtype=torch.float32, device=dev)
    _lib.web_score_grid_fwd_bwd(model.sg, rows(eq), ld_e, rows(edb), ld_e, m, n, model.params,
                                lab, n + pad_lab, m * n, torch.from_numpy(ystats).to(dev),
                                add_label, s if want_s else None, n + pad_s, gq, D + pad_g, gdb,
                                D + pad_g + 1, grad, loss if want_loss else None, ws)
    torch.cuda.synchronize()
    return s, gq, gdb, grad, loss


def _with_qc(qc, fn):
    old = os.environ.get(QC_ENV)
    if qc:
        os.environ[QC_ENV] = str(qc)
    try:
        return fn()
    finally:
        if qc:
            if old is None:
                del os.environ[QC_ENV]
            else:
                os.environ[QC_ENV] = old


@pytest.mark.parametrize('case', GRID_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_web_grid_adjoint_matches_autograd(gpu, case):
    D, K, m, n = case[:4]
    prob, eq, edb, labels, ystats, add_label, ref = _unsaturated_case(case)
    s_ref, l_ref, min_m, min_s, gq_ref, gdb_ref, head_ref = ref
    assert min_m > 1e-3, min_m                      # no relu on its kink
    if case[7] == 'relu':
        assert min_s > 1e-6, min_s
    assert np.abs(gq_ref).max() > 1e-9 and np.abs(gdb_ref).max() > 1e-9
    model = gpu_model(prob, gpu)
    assert model.is_web and model.web_embed_dim == D
    s, gq, gdb, grad, loss = _with_qc(case[8], lambda: _run_grid(model, eq, edb, labels, ystats,
                                                                 add_label))
    s, gq, gdb = s.cpu().numpy(), gq.cpu().numpy(), gdb.cpu().numpy()
    assert np.all(s[:, n:] == SENTINEL), 'columns j >= n of s_out were written'
    assert np.all(gq[:, D:] == SENTINEL) and np.all(gdb[:, D:] == SENTINEL)
    es = float((np.abs(s[:, :n] - s_ref) / (1.0 + np.abs(s_ref))).max())
    el = abs(float(loss.item()) - l_ref) / (1.0 + abs(l_ref))
    print('D {} K {} {}x{}: s err {:.3g} loss err {:.3g} (loss {:.6g}) min|m_k| {:.3g} '
          'max|s| {:.3g}'.format(D, K, m, n, es, el, l_ref, min_m, float(np.abs(s_ref).max())))
    assert es <= TOL, es
    assert el <= TOL, (float(loss.item()), l_ref)
    _block_close(gq[:, :D], gq_ref, 'g_emb_q')
    _block_close(gdb[:, :D], gdb_ref, 'g_emb_db')
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


# ---- 2. contract --------------------------------------------------------------------------
def _contract_inputs(gpu, D=68, K=10, m=9, n=130):
    prob, _ = _head_problem(D, K, 'reference', 'broadcast', True, 'gaussian')
    eq, edb, labels, ystats = _draw(D, m, n, 5)
    return gpu_model(prob, gpu), eq, edb, labels, ystats


@pytest.mark.parametrize('qc', [0, 4])
def test_web_grid_scores_are_bitwise_the_retrieval_grid(gpu, qc):
    import torch
    model, eq, edb, labels, ystats = _contract_inputs(gpu)
    n = edb.shape[0]
    s = _with_qc(qc, lambda: _run_grid(model, eq, edb, labels, ystats, True))[0]
    want = model.web_score_grid(torch.from_numpy(eq).to(gpu), torch.from_numpy(edb).to(gpu),
                                final=False)
    assert torch.equal(s[:, :n], want)


@pytest.mark.parametrize('qc', [0, 4])
def test_web_grid_is_bitwise_deterministic_and_stride_independent(gpu, qc):
    """Three column blocks, several forward workgroups per block and (qc = 4) three query
    chunks: every cross-workgroup sum and every accumulation over chunks is exercised.  The
    strided rows of sg_web_embed (ld = 128) and contiguous [n][D] rows give the same bits, and
    so do calls without s_out and loss_out."""
    import torch
    model, eq, edb, labels, ystats = _contract_inputs(gpu)
    a = _with_qc(qc, lambda: _run_grid(model, eq, edb, labels, ystats, True))
    b = _with_qc(qc, lambda: _run_grid(model, eq, edb, labels, ystats, True))
    c = _with_qc(qc, lambda: _run_grid(model, eq, edb, labels, ystats, True, ld_e=128))
    d = _with_qc(qc, lambda: _run_grid(model, eq, edb, labels, ystats, True, want_s=False,
                                       want_loss=False))
    names = ('s', 'g_emb_q', 'g_emb_db', 'grad', 'loss')
    for x, y, z, what in zip(a, b, c, names):
        assert torch.equal(x, y), what
        assert torch.equal(x, z), what + ' (strided rows)'
    for i in (1, 2, 3):
        assert torch.equal(a[i], d[i]), names[i] + ' (no s_out, no loss_out)'
    assert bool((d[0] == SENTINEL).all()) and float(d[4].item()) == SENTINEL
    head0 = _offsets(_head_problem(68, 10, 'reference', 'broadcast', True, 'gaussian')[0])[0][
        (4, 'weights_W')][0]
    g = a[3]
    assert bool((g[:head0] == SENTINEL).all()) and float(g[head0:].abs().max().item()) > 0
    assert not bool((g[head0:] == SENTINEL).any())       # the whole head range was written
    D, n = eq.shape[1], edb.shape[0]
    assert bool((a[0][:, n:] == SENTINEL).all())
    assert bool((a[1][:, D:] == SENTINEL).all()) and bool((a[2][:, D:] == SENTINEL).all())
    # chunking does not change the scores, and the other outputs only by summation order
    if qc:
        for x, y, what in zip(a, _run_grid(model, eq, edb, labels, ystats, True), names):
            if what == 's':
                assert torch.equal(x, y)
            else:
                scale = float(y[y != SENTINEL].abs().max().item())
                assert float((x - y).abs().max().item()) <= 1e-5 * scale, what
    # Columns k >= K of the tables: web_grid_q_kernel loads no parameter for them (its loads
    # are masked by c < K), so they are zero whatever the parameters hold, and the forward
    # kernel masks them again (GridCol.mask).  No parameter is read only by them: a
    # perturbation test would be vacuous.


# ---- 3. sg_web_embed_bwd against the oracle's _node_backward ------------------------------
def _oracle_embed_bwd(prob, idx, g_emb):
    """Σ_c _node_backward of graph idx[c] seeded with g_emb[c][:D] (entries with idx < 0 are
    skipped).  The backward is linear in its seed, so the seeds of a graph's entries are
    summed in float64 and each distinct graph is walked once."""
    spec = prob.oracle_spec()
    P = O.unflatten(spec, prob.params.astype(np.float64))
    G = {k: np.zeros_like(v) for k, v in P.items()}
    gs = oracle_graphs(prob)
    seeds = {}
    for c, gi in enumerate(idx):
        if gi >= 0:
            seeds[int(gi)] = seeds.get(int(gi), 0.0) + np.asarray(g_emb[c], np.float64)
    for gi, seed in sorted(seeds.items()):
        x, caches = O._node_forward(spec, P, gs[gi], 0, 0, 0)
        O._node_backward(spec, P, G, gs[gi], caches, seed[:np.size(x)].reshape(np.shape(x)))
    return O.flatten(spec, G)


def _run_embed_bwd(model, store, idx, g_emb, gpu):
    import torch
    from graphembedding_amd import _lib
    count = len(idx)
    idx_t = None if idx is None else torch.as_tensor(np.asarray(idx, np.int64), dtype=torch.int32,
                                                     device=gpu)
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(_lib.web_embed_bwd_workspace_bytes(model.sg, count) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    g = torch.from_numpy(np.ascontiguousarray(g_emb)).to(gpu)
    _lib.web_embed_bwd(model.sg, store.to_device(gpu), idx_t, count, model.params, g,
                       g_emb.shape[1], grad, ws, status)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), int(status.item())


def _check_node_range(prob, got, want, what):
    offs, total = _offsets(prob)
    head0 = offs[(len(prob.layers) - 1, 'weights_W')][0]
    assert np.all(got[head0:] == SENTINEL), 'the head range of grad_out was written'
    assert not np.any(got[:head0] == SENTINEL)
    full = got.copy()
    full[head0:] = 0.0
    assert not want[head0:].any()
    print(check_grad_per_var(full, want, prob.layers, prob.d_in, TOL, what))


@pytest.mark.parametrize('name', ['d64', 'd50', 'd512_k16'])
def test_web_embed_bwd_matches_oracle(gpu, name):
    from graphembedding_amd import _lib
    prob, model, store, _ = _case(name, gpu)
    G, D, ld = len(store), model.web_embed_dim, _lib.web_embed_ld(model.sg)
    rng = np.random.default_rng(17)
    for count in (1, 7, 300):
        idx = rng.integers(0, G, size=count)                 # with repeats
        idx[:min(count, 4)] = rng.permutation(4)[:min(count, 4)]
        # rows of stride ld (what web_grid_fwd_bwd passes) and, for the odd count, of stride D
        width = D if count == 7 else ld
        g_emb = rng.standard_normal((count, width)).astype(np.float32)
        got, st = _run_embed_bwd(model, store, idx, g_emb, gpu)
        assert st == 0
        _check_node_range(prob, got, _oracle_embed_bwd(prob, idx, g_emb[:, :D]),
                          '{} count {}'.format(name, count))
        again, _ = _run_embed_bwd(model, store, idx, g_emb, gpu)
        assert np.array_equal(got, again)                    # bitwise on one device
    # graph_idx = NULL: graphs 0 .. count-1
    g_emb = rng.standard_normal((G, ld)).astype(np.float32)
    import torch
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=gpu)
    ws = torch.empty(_lib.web_embed_bwd_workspace_bytes(model.sg, G) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    _lib.web_embed_bwd(model.sg, store.to_device(gpu), None, G, model.params,
                       torch.from_numpy(g_emb).to(gpu), ld, grad, ws, None)
    _check_node_range(prob, grad.cpu().numpy(), _oracle_embed_bwd(prob, range(G), g_emb[:, :D]),
                      name + ' all graphs')


def test_web_embed_bwd_status_and_zero_contribution(gpu):
    from graphembedding_amd import _lib
    prob, model, store, _ = _case('d64', gpu)
    ld = _lib.web_embed_ld(model.sg)
    g_emb = np.random.default_rng(23).standard_normal((5, ld)).astype(np.float32)
    for idx in ([0, 10_000, 2, 3, 4], [10_000, -5, 1, 2, 3]):
        got, st = _run_embed_bwd(model, store, idx, g_emb, gpu)
        assert st == _lib.SG_ERR_ARG
        kept = [i if 0 <= i < len(store) else -1 for i in idx]
        _check_node_range(prob, got, _oracle_embed_bwd(prob, kept, g_emb[:, :64]), str(idx))
    # count = 0 zeroes the node-layer range and nothing else
    got, st = _run_embed_bwd(model, store, [], np.zeros((0, ld), np.float32), gpu)
    head0 = _offsets(prob)[0][(4, 'weights_W')][0]
    assert st == 0 and not got[:head0].any() and np.all(got[head0:] == SENTINEL)


# ---- 4. end to end against the pairwise path ---------------------------------------------
E2E = {   # name: (node counts, D, K, node types)
    'd64': ([1, 15, 16, 17, 63, 64, 9, 33, 40, 5, 22, 50], 64, 10, 29),
    'd512_k16': ([1, 130, 257, 496, 511, 512], 512, 16, 60),
}
_E2E_CACHE = {}


def _e2e(name):
    if name not in _E2E_CACHE:
        counts, D, K, n_types = E2E[name]
        _E2E_CACHE[name] = _alive(sized_problem(counts, ntn_stack(D, K, dropout=0.0), n_max=D,
                                                seed=31, n_types=n_types))
    return _E2E_CACHE[name]


def _pairwise_batch(model, store, q, db, labels):
    import torch
    pairs = np.stack([np.repeat(q, len(db)), np.tile(db, len(q))], axis=1).astype(np.int32)
    pi = torch.from_numpy(pairs).to(model.params.device)
    return model.web_batch(store, pi, labels.reshape(-1).copy(), batch_total=len(pairs))


def _grids(G):
    """q_idx x db_idx with overlap and repeats, and the identity grid."""
    return {'overlap': (np.array([0, 2, 2, G - 1, 1]), np.array([1, 2, 3, 3, 0, G - 1, 4])),
            'identity': (None, None)}


@pytest.mark.parametrize('grid', ['overlap', 'identity'])
@pytest.mark.parametrize('name', list(E2E))
def test_web_grid_fwd_bwd_matches_pairwise(gpu, name, grid):
    import torch
    prob = _e2e(name)
    model = gpu_model(prob, gpu)
    assert model.is_web and model.sg.keep_prob == 1.0
    store = _csr(prob, model)
    G = len(store)
    q, db = _grids(G)[grid]
    qa = np.arange(G) if q is None else q
    da = np.arange(G) if db is None else db
    labels = np.random.default_rng(2).uniform(0.05, 1.0, size=(len(qa), len(da))).astype(np.float32)
    s = torch.empty((len(qa), len(da)), dtype=torch.float32, device=gpu)
    gp = model.web_grid_fwd_bwd(store, labels, q, db, s_out=s)
    gp.check()
    assert gp.identity == (grid == 'identity')
    g_grid = model.grad.cpu().numpy().copy()
    l_grid = float(model.loss_buf[0].item())
    batch = _pairwise_batch(model, store, qa, da, labels)
    s_pair = torch.empty(batch.n_pairs, dtype=torch.float32, device=gpu)
    model.fwd_bwd(batch, seed=0, s_out=s_pair)
    g_pair = model.grad.cpu().numpy().copy()
    l_pair = float(model.loss_buf[0].item())
    print(name, grid, 'loss grid', l_grid, 'pairwise', l_pair)
    assert abs(l_grid - l_pair) <= TOL * abs(l_pair), (l_grid, l_pair)
    assert float(np.abs(g_pair).max()) > 0
    print(check_grad_per_var(g_grid, g_pair, prob.layers, prob.d_in, TOL, 'grid vs pairwise'))
    np.testing.assert_allclose(s.cpu().numpy().reshape(-1), s_pair.cpu().numpy(), rtol=TOL,
                               atol=TOL)
    # a problem built once gives the same bits again
    model.web_grid_fwd_bwd(gp)
    assert np.array_equal(model.grad.cpu().numpy(), g_grid)


def test_three_web_grid_train_steps_match_pairwise_adam(gpu):
    prob = _e2e('d64')
    a, b = gpu_model(prob, gpu), gpu_model(prob, gpu)
    store = _csr(prob, a)
    q, db = _grids(len(store))['overlap']
    labels = np.random.default_rng(2).uniform(0.05, 1.0, size=(len(q), len(db))).astype(np.float32)
    gp = a.web_grid_problem(store, labels, q, db)
    batch = _pairwise_batch(b, store, q, db, labels)
    for step in range(3):
        la = a.web_grid_train_step(gp)
        lb = b.train_step(batch, seed=0)
        assert abs(la - lb) <= TOL * max(1.0, abs(lb)), (step, la, lb)
    gp.check()
    assert a.step_count == b.step_count == 3
    err = float((a.params - b.params).abs().max().item())
    moved = float((a.params - a.torch.from_numpy(prob.params).to(gpu)).abs().max().item())
    print('max |param diff| after 3 steps', err, 'moved', moved)
    assert moved > 1e-3
    assert err <= 1e-4, err


# ---- 5. refusal ---------------------------------------------------------------------------
def test_web_grid_training_refusals(gpu):
    from graphembedding_amd import _lib
    prob = _e2e('d64')
    store_model = gpu_model(prob, gpu)
    store = _csr(prob, store_model)
    labels = np.full((len(store), len(store)), 0.5, np.float32)
    dropped = gpu_model(prob, gpu, dropout=0.1)
    before = dropped.grad.clone()
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        dropped.web_grid_fwd_bwd(store, labels)
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        dropped.web_grid_train_step(store, labels)
    assert dropped.torch.equal(before, dropped.grad) and dropped.step_count == 0
    # the C ABI refuses on its own, whatever the Python layer checked
    with pytest.raises(_lib.SiameseHipError):
        _lib.web_score_grid_bwd_workspace_bytes(dropped.sg, 4, 4)
    with pytest.raises(_lib.SiameseHipError):
        _lib.web_embed_bwd_workspace_bytes(dropped.sg, 4)
    # the small-D calls keep refusing graph-store models
    with pytest.raises(_lib.SiameseHipError):
        store_model.grid_fwd_bwd(store, labels)
    with pytest.raises(_lib.SiameseHipError):
        store_model.grid_problem(store, labels)
