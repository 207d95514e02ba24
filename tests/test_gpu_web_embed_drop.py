"""Embed-once training with graph-keyed dropout for graph-store (Web) models on the GPU
(include/siamese_web_embed_drop.h): sg_web_embed_drop against the oracle's _node_forward and
head mask, against the masks sg_web_forward draws, its independence of partner, call split and
chunking, sg_web_embed_drop_bwd and web_grid_fwd_bwd(dropout='graph') against a float64
reference built from oracle pieces, invalid entries, and the Python surface (WebAllPairsGrid).
The oracle's node forward covers every layer option of the Web stack (the sparse layer-0 mask,
layers 1 and 2, a non-zero padding_value, the head mask over all D columns), so test 1 checks
all four masks and test 2 ties them to the pair kernel's.
Bars are imported, not restated: embeddings and scores within test_gpu_web_embed.TOL (rtol =
atol), loss and every gradient block within test_gpu_web_embed_train.TOL of its own largest
component.  The 1 / keep <= 2 scaling of the masked tensors does not change their order."""
import types

import numpy as np
import pytest

from _embed_fixtures import gpu_model, ntn_stack, sized_problem
from _fixtures import check_grad_per_var
from oracle import siamese_oracle as O
from test_gpu_embed_drop import _Oracle
from test_gpu_embed_train import _autograd_head, _block_close, _offsets
from test_gpu_web_embed import TOL as EMBED_TOL
from test_gpu_web_embed import _alive, _csr, _pad
from test_gpu_web_embed_train import SENTINEL
from test_gpu_web_embed_train import TOL as TRAIN_TOL
from test_gpu_web_embed_train import _check_node_range, _grids, _run_embed_bwd

pytestmark = pytest.mark.gpu

KEEPS = (0.5, 0.9)
SEED = 0x1234_5678_9ABC
KINK = 1e-3   # the margin of test_gpu_web_embed_train._unsaturated_case

# name: (node counts, D, K, node types, padding_value).  The first six graphs of every case
# are 1, 15, 16, 17, D - 1 and D nodes (d512: 1 .. 512 as test_gpu_web_embed_train's).
CASES = {
    'd64': ([1, 15, 16, 17, 63, 64, 9, 33, 40, 5, 22, 50], 64, 10, 29, 0),
    'd50_pad1': ([1, 15, 16, 17, 49, 50, 33, 8], 50, 10, 29, 1),   # D % 16 != 0, Padding = 1
    'd512_k16': ([1, 130, 257, 496, 511, 512], 512, 16, 60, 0),
}
_CACHE = {}


def _problem(name, keep, **flags):
    counts, D, K, n_types, padv = CASES[name]
    ov = ntn_stack(D, K, layer_3=_pad(D, padv), dropout=round(1.0 - keep, 6), **flags)
    return _alive(sized_problem(counts, ov, n_max=D, seed=31, n_types=n_types))


def _case(name, keep, gpu):
    """Problem, model, CSR store and oracle of a case at a keep probability: built once,
    read only."""
    key = (name, keep)
    if key not in _CACHE:
        prob = _problem(name, keep)
        model = gpu_model(prob, gpu)
        assert model.is_web and model.web_embed_dim == CASES[name][1]
        assert abs(model.sg.keep_prob - keep) < 1e-6
        _CACHE[key] = (prob, model, _csr(prob, model), _Oracle(prob))
    return _CACHE[key]


def _idx_t(idx, gpu):
    import torch
    return torch.as_tensor(np.asarray(idx, np.int64), dtype=torch.int32, device=gpu)


def _embed_drop(model, store, idx, seed, entry_offset=0, dev=None):
    """sg_web_embed_drop into a sentinel-filled buffer: (rows [count][ld] torch, status)."""
    import torch
    from graphembedding_amd import _lib
    gpu = model.params.device
    ld = _lib.web_embed_ld(model.sg)
    out = torch.full((len(idx), ld), 7.0, dtype=torch.float32, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(_lib.web_embed_drop_workspace_bytes(model.sg, len(idx)) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    _lib.web_embed_drop(model.sg, dev or store.to_device(gpu), _idx_t(idx, gpu), len(idx),
                        entry_offset, model.params, seed, out, ws, status)
    torch.cuda.synchronize()
    return out, int(status.item())


def _embed_plain(model, store, idx):
    """sg_web_embed: rows [count][ld] torch."""
    import torch
    from graphembedding_amd import _lib
    gpu = model.params.device
    out = torch.full((len(idx), _lib.web_embed_ld(model.sg)), 7.0, dtype=torch.float32,
                     device=gpu)
    ws = torch.empty(_lib.web_embed_workspace_bytes(model.sg, len(idx)) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    _lib.web_embed(model.sg, store.to_device(gpu), _idx_t(idx, gpu), len(idx), model.params, out,
                   ws, None)
    torch.cuda.synchronize()
    return out


def _embed_drop_bwd(model, store, idx, seed, g_emb, entry_offset=0, dev=None):
    """sg_web_embed_drop_bwd: (grad_out with a sentinel in the head range, status)."""
    import torch
    from graphembedding_amd import _lib
    gpu = model.params.device
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(_lib.web_embed_drop_bwd_workspace_bytes(model.sg, len(idx)) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    g = torch.from_numpy(np.ascontiguousarray(g_emb, np.float32)).to(gpu)
    _lib.web_embed_drop_bwd(model.sg, dev or store.to_device(gpu), _idx_t(idx, gpu), len(idx),
                            entry_offset, model.params, seed, g, g_emb.shape[1], grad, ws, status)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), int(status.item())


def _entries(G, count, seed):
    """The six graphs of the special node counts first, then random ones (with repeats)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[3, 0, 2, 1, 5, 4], rng.integers(0, G, size=count)])[:count]


# ---- 1. forward against the oracle -------------------------------------------------------
@pytest.mark.parametrize('count', [5, 67])   # an odd tail each; 67: more units than one workgroup
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('name', list(CASES))
def test_web_embed_drop_matches_oracle(gpu, name, keep, count):
    prob, model, store, orc = _case(name, keep, gpu)
    D, padv = CASES[name][1], CASES[name][4]
    idx = _entries(len(store), count, count)
    got, st = _embed_drop(model, store, idx, SEED)
    assert st == 0
    got = got.cpu().numpy()
    want = orc.rows(idx, SEED)
    assert want.shape == (count, D)
    print(name, keep, count, 'max |emb - oracle|', float(np.abs(got[:, :D] - want).max()),
          'zeros', float((want == 0).mean()))
    np.testing.assert_allclose(got[:, :D], want, rtol=EMBED_TOL, atol=EMBED_TOL)
    assert not got[:, D:].any()                          # columns [D, ld) zero
    if padv:
        # the layer-4 mask on the Padding columns [N, D): entry 1 is the one-node graph
        pad = got[1, 1:D]
        assert set(np.unique(pad)) == {0.0, np.float32(padv / np.float32(keep))}
        assert np.array_equal(pad != 0, want[1, 1:] != 0)


# ---- 2. the masks of the pair kernel -----------------------------------------------------
@pytest.mark.parametrize('keep', KEEPS)
def test_web_embed_drop_draws_the_pair_kernels_masks(gpu, keep):
    """Pair q = (g_2q, g_2q+1) through sg_web_forward (dropout on, pair_offset 0) against grid
    entry (2 q, 2 q + 1) of sg_web_score_grid on the masked embeddings with the keep-1 copy of
    the model, under the same seed.  The eight pairs mix the three size classes (at most 16,
    at most 32, more nodes)."""
    import torch
    from graphembedding_amd import _lib
    prob, model, store, _ = _case('d64', keep, gpu)
    ids = np.array([0, 5, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 5, 0, 4, 1])
    npair, n = 8, 16
    pairs = torch.from_numpy(ids.reshape(npair, 2).astype(np.int32)).to(gpu)
    batch = model.web_batch(store, pairs, np.zeros(npair, np.float32))
    assert batch.pair_offset == 0
    fwd = model.pred_sim_without_act(batch, seed=SEED).cpu().numpy().reshape(-1)
    other = model.pred_sim_without_act(batch, seed=SEED + 1).cpu().numpy().reshape(-1)
    emb, st = _embed_drop(model, store, ids, SEED)
    assert st == 0
    keep1 = model._sg_keep1()
    assert keep1.keep_prob == 1.0
    ld = int(emb.shape[1])
    ws = torch.empty(_lib.web_score_grid_workspace_bytes(keep1, n) // 4 + 1, dtype=torch.float32,
                     device=gpu)
    out = torch.empty((n, n), dtype=torch.float32, device=gpu)
    _lib.web_score_grid(keep1, emb, ld, emb, ld, n, n, model.params, False, out, n, ws)
    out = out.cpu().numpy()
    got = np.array([out[2 * q, 2 * q + 1] for q in range(npair)])
    print(keep, 'max |grid - pair|', float(np.abs(got - fwd).max()), 'other seed',
          float(np.abs(other - fwd).max()))
    assert np.abs(other - fwd).max() > 10 * EMBED_TOL     # the masks matter to these scores
    np.testing.assert_allclose(got, fwd, rtol=EMBED_TOL, atol=EMBED_TOL)
    if keep == 0.5:
        # the masks are on: entries that are positive in sg_web_embed's rows are zero here
        plain = _embed_plain(model, store, ids)
        assert not torch.equal(plain, emb)
        assert int(((plain > 0) & (emb == 0)).sum().item()) > 0
        assert int(((plain > 0) & (emb > 0)).sum().item()) > 0


# ---- 3. independence of split, partner and chunk -----------------------------------------
def test_web_embed_drop_rows_do_not_depend_on_split_or_partner(gpu):
    import torch
    prob, model, store, _ = _case('d64', 0.5, gpu)
    G = len(store)
    idx = np.random.default_rng(9).integers(0, G, size=1027)
    whole, st = _embed_drop(model, store, idx, SEED)
    assert st == 0
    # (a) the same entries issued as several calls with even entry_offsets
    for a, b in ((0, 4), (4, 512), (512, 1024), (1024, 1027), (4, 8)):
        part, st = _embed_drop(model, store, idx[a:b], SEED, entry_offset=a)
        assert st == 0 and torch.equal(part, whole[a:b]), (a, b)
    # the entry number counts, not the position in the call
    shifted, _ = _embed_drop(model, store, idx[4:8], SEED, entry_offset=0)
    assert not torch.equal(shifted, whole[4:8])
    # (b) other partners in the unit, other size classes in the workgroups
    other = idx.copy()
    other[1::2] = (idx[1::2] + 1 + np.arange(len(idx[1::2])) % (G - 1)) % G
    assert not np.any(other[1::2] == idx[1::2])
    rows, _ = _embed_drop(model, store, other, SEED)
    assert torch.equal(rows[0::2], whole[0::2]) and not torch.equal(rows[1::2], whole[1::2])
    other = idx.copy()
    other[0::2] = (idx[0::2] + 1 + np.arange(len(idx[0::2])) % (G - 1)) % G
    rows, _ = _embed_drop(model, store, other, SEED)
    assert torch.equal(rows[1::2], whole[1::2])


def test_web_embed_drop_bwd_crosses_its_chunk_boundary(gpu):
    """(c) 1,027 entries: the backward's second chunk starts at entry 1,024."""
    prob, model, store, _ = _case('d64', 0.5, gpu)
    rng = np.random.default_rng(10)
    idx = rng.integers(0, len(store), size=1027)
    g_emb = rng.standard_normal((1027, 128)).astype(np.float32)
    whole, st = _embed_drop_bwd(model, store, idx, SEED, g_emb)
    again, _ = _embed_drop_bwd(model, store, idx, SEED, g_emb)
    assert st == 0 and np.array_equal(whole, again)          # bitwise on one device
    a, sa = _embed_drop_bwd(model, store, idx[:1024], SEED, g_emb[:1024])
    b, sb = _embed_drop_bwd(model, store, idx[1024:], SEED, g_emb[1024:], entry_offset=1024)
    assert sa == 0 and sb == 0
    head0 = _offsets(prob)[0][(4, 'weights_W')][0]
    want = np.zeros_like(whole, dtype=np.float64)
    want[:head0] = a[:head0].astype(np.float64) + b[:head0].astype(np.float64)
    assert np.abs(b[:head0]).max() > 0
    _check_node_range(prob, whole, want, '1027 entries vs 1024 + 3')
    # the tail under entry_offset 0 is another gradient: the entry numbers reach the chunk
    c, _ = _embed_drop_bwd(model, store, idx[1024:], SEED, g_emb[1024:], entry_offset=0)
    assert not np.array_equal(b, c)


# ---- 4. keep = 1 and no dropout flag -----------------------------------------------------
def _no_flag_problem():
    """flags.dropout = 0.5 with every layer's dropout flag off."""
    ov = dict(layer_0='GraphConvolution:output_dim=32,act=relu,dropout=False,bias=True,'
                      'sparse_inputs=True',
              layer_1='GraphConvolution:input_dim=32,output_dim=16,act=identity,dropout=False,'
                      'bias=True,sparse_inputs=False',
              layer_2='Dense:input_dim=16,output_dim=1,dropout=False,act=relu,bias=True',
              layer_4='NTN:input_dim=64,feature_map_dim=10,inneract=relu,dropout=False,bias=True')
    return _problem('d64', 0.5, **ov)


@pytest.mark.parametrize('which', ['keep1', 'no_flag'])
def test_web_embed_drop_without_effective_dropout_is_web_embed(gpu, which):
    import torch
    prob = _problem('d64', 1.0) if which == 'keep1' else _no_flag_problem()
    model = gpu_model(prob, gpu)
    assert model.is_web and (model.sg.keep_prob == 1.0) == (which == 'keep1')
    store = _csr(prob, model)
    idx = _entries(len(store), 67, 4)
    ref = _embed_plain(model, store, idx)
    g_emb = np.random.default_rng(5).standard_normal((67, ref.shape[1])).astype(np.float32)
    want, st = _run_embed_bwd(model, store, idx, g_emb, gpu)
    assert st == 0
    for seed, off in ((SEED, 0), (SEED + 1, 6)):
        got, st = _embed_drop(model, store, idx, seed, entry_offset=off)
        assert st == 0 and torch.equal(got, ref)
        grad, st = _embed_drop_bwd(model, store, idx, seed, g_emb, entry_offset=off)
        assert st == 0 and np.array_equal(grad, want)


# ---- 5. backward against the oracle ------------------------------------------------------
def _oracle_drop_bwd(orc, idx, g_emb, seed, entry_offset=0):
    """Σ_c _node_backward of entry c on its masked caches, seeded with mask · g_emb[c] / keep
    (entries with idx < 0 are skipped)."""
    G = {k: np.zeros_like(v) for k, v in orc.P.items()}
    for c, gi in enumerate(idx):
        if gi < 0:
            continue
        _, m, caches, shape = orc.entry(int(gi), entry_offset + c, seed)
        gx = np.where(m, np.asarray(g_emb[c][:m.size], np.float64) / orc.keep, 0.0)
        O._node_backward(orc.spec, orc.P, G, orc.gs[int(gi)], caches, gx.reshape(shape))
    return O.flatten(orc.spec, G)


@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('name', list(CASES))
def test_web_embed_drop_bwd_matches_oracle(gpu, name, keep):
    from graphembedding_amd import _lib
    prob, model, store, orc = _case(name, keep, gpu)
    D, ld = CASES[name][1], _lib.web_embed_ld(model.sg)
    rng = np.random.default_rng(17)
    for count in ((7,) if D == 512 else (7, 67)):
        idx = _entries(len(store), count, 100 + count)
        # rows of stride ld (what web_grid_fwd_bwd passes) and, for the small count, of stride D
        width = D if count == 7 else ld
        g_emb = rng.standard_normal((count, width)).astype(np.float32)
        got, st = _embed_drop_bwd(model, store, idx, SEED, g_emb)
        assert st == 0
        _check_node_range(prob, got, _oracle_drop_bwd(orc, idx, g_emb, SEED),
                          '{} keep {} count {}'.format(name, keep, count))


# ---- 6. end to end against a float64 reference -------------------------------------------
def _reference_step(prob, orc, q, db, labels, seed):
    """Loss, flat gradient and the smallest |m_k| of web_grid_fwd_bwd(dropout='graph') in
    float64: per distinct graph the oracle's _node_forward under its entry's masks and the head
    mask; the NTN head, loss and adjoint over the m x n block at keep 1
    (test_gpu_embed_train._autograd_head) on the masked embeddings; the role sum;
    g_e = mask · g_x / keep; the oracle's _node_backward."""
    uniq, inv = np.unique(np.concatenate([q, db]), return_inverse=True)
    ent = [orc.entry(int(gi), c, seed) for c, gi in enumerate(uniq)]
    emb = np.stack([e[0] for e in ent])
    qp, dp = inv[:len(q)], inv[len(q):]
    y = labels.astype(np.float64)
    ystats = np.array([y.mean(), 0.5 * ((y - y.mean()) ** 2).sum()])
    s, loss, min_m, _, gq, gdb, head = _autograd_head(prob, emb[qp], emb[dp], labels, ystats, True)
    gx = np.zeros_like(emb)
    np.add.at(gx, qp, gq)
    np.add.at(gx, dp, gdb)
    G = {k: np.zeros_like(v) for k, v in orc.P.items()}
    for c, gi in enumerate(uniq):
        _, m, caches, shape = ent[c]
        O._node_backward(orc.spec, orc.P, G, orc.gs[int(gi)], caches,
                         np.where(m, gx[c] / orc.keep, 0.0).reshape(shape))
    for name, g in head.items():
        G[(orc.hi, name)] = g
    return loss, O.flatten(orc.spec, G), min_m, float(np.abs(s).max())


def _unsaturated_step(name, keep, grid):
    """The case's problem, grid, labels, seed and float64 reference, chosen on the CPU the way
    test_gpu_web_embed_train._unsaturated_case chooses its inputs: U = |U| / K divided by the
    power of two that brings max |s| of the float64 reference to at most 1 (the score is
    linear in U and m_k does not depend on it), and the dropout seed the first for which no
    relu of the head sits within KINK of its kink."""
    prob = _problem(name, keep)
    K = CASES[name][2]
    oU = _offsets(prob)[0][(4, 'weights_U')][0]
    prob.params[oU:oU + K] = np.abs(prob.params[oU:oU + K]) / K
    G = len(prob.mgs)
    q, db = _grids(G)[grid]
    qa = np.arange(G) if q is None else q
    da = np.arange(G) if db is None else db
    labels = np.random.default_rng(2).uniform(0.05, 1.0, size=(len(qa), len(da))).astype(np.float32)
    for seed in range(SEED, SEED + 200):
        loss, g_ref, min_m, smax = _reference_step(prob, _Oracle(prob), qa, da, labels, seed)
        if min_m <= KINK:
            continue
        if smax > 1.0:
            prob.params[oU:oU + K] *= np.float32(2.0 ** -int(np.ceil(np.log2(smax))))
            loss, g_ref, min_m, smax = _reference_step(prob, _Oracle(prob), qa, da, labels, seed)
        return prob, q, db, qa, da, labels, seed, loss, g_ref, min_m, smax
    raise AssertionError('no seed keeps every m_k clear of the relu kink')


@pytest.mark.parametrize('grid', ['overlap', 'identity'])
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('name', ['d64', 'd512_k16'])
def test_web_grid_fwd_bwd_graph_dropout_matches_reference(gpu, name, keep, grid):
    prob, q, db, qa, da, labels, seed, l_ref, g_ref, min_m, smax = _unsaturated_step(
        name, keep, grid)
    assert min_m > KINK and smax <= 1.0, (min_m, smax)   # conditions on the inputs, met on the CPU
    model = gpu_model(prob, gpu)
    store = _csr(prob, model)
    assert len(store) == (12 if name == 'd64' else 6)
    gp = model.web_grid_fwd_bwd(store, labels, q, db, dropout='graph', seed=seed)
    gp.check()
    assert gp.dropout == 'graph' and gp.identity == (grid == 'identity')
    g_gpu = model.grad.cpu().numpy().copy()
    l_gpu = float(model.loss_buf[0].item())
    print(name, keep, grid, 'seed', seed - SEED, 'loss', l_gpu, 'reference', l_ref,
          'min |m_k|', min_m, 'max |s|', smax)
    assert abs(l_gpu - l_ref) <= TRAIN_TOL * max(1.0, abs(l_ref)), (l_gpu, l_ref)
    print(check_grad_per_var(g_gpu, g_ref, prob.layers, prob.d_in, TRAIN_TOL,
                             'graph dropout vs float64 reference'))
    # the masks matter: another seed's reference gradient is far outside the bar
    _, g_other, _, _ = _reference_step(prob, _Oracle(prob), qa, da, labels, seed + 1)
    assert np.abs(g_other - g_ref).max() > 10 * TRAIN_TOL * np.abs(g_ref).max()
    # a problem built once gives the same bits again under the same seed
    model.web_grid_fwd_bwd(gp, seed=seed)
    assert np.array_equal(model.grad.cpu().numpy(), g_gpu)


# ---- 7. status ---------------------------------------------------------------------------
def test_web_embed_drop_invalid_entries(gpu):
    """An id outside the store (SG_ERR_ARG) and a node count above the store's n_max
    (SG_ERR_SHAPE): zero rows, nothing in the gradient, and the other entries, at the same
    entry numbers, are bitwise those of a call without the bad entries."""
    import torch
    from graphembedding_amd import _lib
    prob, model, store, _ = _case('d64', 0.5, gpu)
    good_idx = [3, 0, 2, 1, 6, 9, 10]                     # 17, 1, 16, 15, 9, 5, 22 nodes
    good, st = _embed_drop(model, store, good_idx, SEED)
    assert st == 0
    out, st = _embed_drop(model, store, [3, 10_000, 2, 1, 6, -1, 10], SEED)
    assert st == _lib.SG_ERR_ARG
    assert not out[1].any() and not out[5].any()
    assert torch.equal(out[[0, 2, 3, 4, 6]], good[[0, 2, 3, 4, 6]])
    # the same device arrays behind a struct that admits 40 nodes: graphs 4 and 5 (63, 64) are
    # too large for it
    store.to_device(gpu)
    small = _lib.csr_struct(len(store), 40, *store._dev, max_nnz=store.max_nnz)
    good40, st = _embed_drop(model, store, good_idx, SEED, dev=small)
    assert st == 0
    out, st = _embed_drop(model, store, [3, 0, 4, 5, 6, 9, 10], SEED, dev=small)
    assert st == _lib.SG_ERR_SHAPE and not out[2:4].any()
    assert torch.equal(out[[0, 1, 4, 5, 6]], good40[[0, 1, 4, 5, 6]])
    # the gradient: the bad unit (entries 2 and 3) adds nothing
    g_emb = np.random.default_rng(6).standard_normal((7, 128)).astype(np.float32)
    for bad, code, dev in (([3, 0, 10_000, -5, 6, 9, 10], _lib.SG_ERR_ARG, None),
                           ([3, 0, 4, 5, 6, 9, 10], _lib.SG_ERR_SHAPE, small)):
        got, st = _embed_drop_bwd(model, store, bad, SEED, g_emb, dev=dev)
        assert st == code
        a, sa = _embed_drop_bwd(model, store, bad[:2], SEED, g_emb[:2], dev=dev)
        b, sb = _embed_drop_bwd(model, store, bad[4:], SEED, g_emb[4:], entry_offset=4, dev=dev)
        assert sa == 0 and sb == 0
        head0 = _offsets(prob)[0][(4, 'weights_W')][0]
        want = np.zeros_like(got, dtype=np.float64)
        want[:head0] = a[:head0].astype(np.float64) + b[:head0].astype(np.float64)
        assert np.abs(want[:head0]).max() > 1e-3
        _check_node_range(prob, got, want, 'bad unit, status {}'.format(code))


# ---- 8. the Python surface ---------------------------------------------------------------
def test_web_grid_dropout_python_surface(gpu):
    from graphembedding_amd import _lib
    prob, _, store, _ = _case('d64', 0.9, gpu)
    model = gpu_model(prob, gpu, learning_rate=0.0, weight_decay=0.0)
    assert model.flags.dropout == pytest.approx(0.1)
    q, db = np.arange(5), np.arange(3, 12)
    labels = np.random.default_rng(8).uniform(0.05, 1.0, size=(5, 9)).astype(np.float32)
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.web_grid_problem(store, labels, q, db)              # dropout=None: today's refusal
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.web_grid_fwd_bwd(store, labels, q, db)
    for bad in ('pair', 'Graph', True, 0.1):
        with pytest.raises(_lib.SiameseHipError, match="None or 'graph'"):
            model.web_grid_problem(store, labels, q, db, dropout=bad)
        with pytest.raises(_lib.SiameseHipError, match="None or 'graph'"):
            model.web_grid_fwd_bwd(store, labels, q, db, dropout=bad)
        with pytest.raises(_lib.SiameseHipError, match="None or 'graph'"):
            model.web_grid_train_step(store, labels, q, db, dropout=bad)
    gp = model.web_grid_problem(store, labels, q, db, dropout='graph')
    assert gp.dropout == 'graph' and model.step_count == 0
    # Adam with a zero learning rate moves nothing: two steps differ by their masks alone
    before = model.params.clone()
    l0 = model.web_grid_train_step(gp)
    l1 = model.web_grid_train_step(gp)
    gp.check()
    assert model.step_count == 2
    assert model.torch.equal(model.params, before)
    assert l0 != l1, (l0, l1)
    model.step_count = 0
    assert model.web_grid_train_step(gp) == l0                    # the same step: the same loss
    # a stored-problem mismatch raises
    plain = gpu_model(prob, gpu, dropout=0.0)
    gp_none = plain.web_grid_problem(store, labels, q, db)
    assert gp_none.dropout is None
    with pytest.raises(_lib.SiameseHipError, match='built with'):
        plain.web_grid_fwd_bwd(gp_none, dropout='graph')
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.web_grid_fwd_bwd(gp_none)                           # a None problem, dropout on
    # dropout='graph' at flags.dropout = 0 is dropout=None, bit for bit
    plain.web_grid_fwd_bwd(gp_none)
    g_none, l_none = plain.grad.clone(), float(plain.loss_buf[0].item())
    assert float(g_none.abs().max().item()) > 0
    plain.web_grid_fwd_bwd(store, labels, q, db, dropout='graph')
    assert float(plain.loss_buf[0].item()) == l_none
    assert plain.torch.equal(plain.grad, g_none)


def test_web_all_pairs_grid(gpu):
    from graphembedding_amd.web import WebAllPairs, WebAllPairsGrid
    prob = _problem('d64', 1.0)
    gs = types.SimpleNamespace(graphs=prob.graphs[:10], mgs=prob.mgs[:10], d_in=prob.d_in)
    labels = np.random.default_rng(3).uniform(0.05, 1.0, size=(10, 10)).astype(np.float32)
    # dropout 0: the loss and gradient of WebAllPairs' batch through fwd_bwd
    model = gpu_model(prob, gpu)
    grid = WebAllPairsGrid(gs, labels, gpu)
    assert len(grid.store) == 10 and grid.total == 100 and grid.dropout is None
    grid.fwd_bwd(model)
    gp = grid.problem(model)
    gp.check()
    assert gp.identity and grid.problem(model) is gp              # cached per model
    g_grid, l_grid = model.grad.cpu().numpy().copy(), float(model.loss_buf[0].item())
    pairs = WebAllPairs(gs, labels, device=gpu, n_cap=model.n_max)
    model.fwd_bwd(pairs.batch(model), seed=0)
    g_pair, l_pair = model.grad.cpu().numpy().copy(), float(model.loss_buf[0].item())
    print('all pairs: loss grid', l_grid, 'pairwise', l_pair)
    assert abs(l_grid - l_pair) <= TRAIN_TOL * abs(l_pair), (l_grid, l_pair)
    assert float(np.abs(g_pair).max()) > 0
    print(check_grad_per_var(g_grid, g_pair, prob.layers, prob.d_in, TRAIN_TOL,
                             'WebAllPairsGrid vs WebAllPairs'))
    # a CsrStore is taken as it is; another model gets a problem of its own
    taken = WebAllPairsGrid(grid.store, labels, gpu)
    assert taken.store is grid.store
    other = gpu_model(prob, gpu)
    assert grid.problem(other) is not gp
    # dropout='graph': three steps, the parameters of three web_grid_train_step calls
    dprob = _problem('d64', 0.9)
    a, b = gpu_model(dprob, gpu), gpu_model(dprob, gpu)
    dgrid = WebAllPairsGrid(gs, labels, gpu, dropout='graph')
    gpb = b.web_grid_problem(dgrid.store, labels, dropout='graph')
    for step in range(3):
        la = dgrid.train_step(a)
        lb = b.web_grid_train_step(gpb)
        assert np.isfinite(la) and la == lb, (step, la, lb)
    dgrid.problem(a).check()
    assert dgrid.problem(a).dropout == 'graph' and a.step_count == b.step_count == 3
    assert a.torch.equal(a.params, b.params)
    moved = float((a.params - a.torch.from_numpy(dprob.params).to(gpu)).abs().max().item())
    assert moved > 1e-3, moved
