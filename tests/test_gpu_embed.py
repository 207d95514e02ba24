"""Embed-once retrieval on the GPU (include/siamese_embed.h): graph embeddings against
the oracle's node stack, the NTN score grid against sg_forward of a keep_prob = 1 model
and against the oracle's pair forward, top-k against numpy lexsort, and the wiring
through train.test and EmbeddingIndex.
Tolerance: the project's per-pair 1e-4 (test_gpu_parity.TOL), rtol = atol."""
import numpy as np
import pytest

from _embed_fixtures import (ATTENTION_STACK, DENSE_AFTER_PAD, gpu_model, ntn_stack,
                             oracle_graphs, sized_problem)
from _fixtures import AVERAGE_STACK
from oracle import siamese_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4

EMBED_STACKS = {   # name: (flag overrides, n_max = Padding dim)
    'default': ({}, 10),
    'average': (AVERAGE_STACK, 10),
    'attention': (ATTENTION_STACK, 10),
    'dense_after_pad': (DENSE_AFTER_PAD, 10),
    'pad30_nmax32': ({}, 30),
}
COUNTS = (1, 7, 64, 531)   # one graph, an odd tail, a full launch, many workgroups


def _node_counts(pd, extra=16, seed=3):
    """1, 8, 9 and the Padding dim, then random counts."""
    rng = np.random.default_rng(seed)
    return [1, 8, 9, pd] + [int(x) for x in rng.integers(1, pd + 1, size=extra)]


def _oracle_embeddings(prob):
    """O._node_forward of every graph at dropout 0, flattened: [G][E] float64."""
    spec = prob.oracle_spec()
    assert spec.keep_prob == 1.0
    P = O.unflatten(spec, prob.params.astype(np.float64))
    return np.stack([np.asarray(O._node_forward(spec, P, g, 0, 0, 0)[0]).reshape(-1)
                     for g in oracle_graphs(prob)])


def _store(prob, model):
    from graphembedding_amd.packer import GraphStore
    return GraphStore(prob.mgs, model.n_max, prob.d_in)


_EMBED_CACHE = {}


def _embed_case(name, gpu):
    """Problem, model, store and oracle embeddings of a stack: built once, read only."""
    if name not in _EMBED_CACHE:
        ov, pd = EMBED_STACKS[name]
        prob = sized_problem(_node_counts(pd), dict(ov, dropout=0.0), n_max=pd, seed=11)
        model = gpu_model(prob, gpu)
        _EMBED_CACHE[name] = (prob, model, _store(prob, model), _oracle_embeddings(prob))
    return _EMBED_CACHE[name]


@pytest.mark.parametrize('name', list(EMBED_STACKS))
def test_embeddings_match_oracle(gpu, name):
    prob, model, store, ref = _embed_case(name, gpu)
    if name == 'pad30_nmax32':
        assert model.n_max == 32 and model.max_nodes == 30
    assert {1, 8, 9, model.max_nodes or 10} <= set(int(x) for x in store.n)
    assert model.embed_dim == ref.shape[1]
    G = len(store)
    all_e = model.embed(store).cpu().numpy()            # graph_idx = None: every graph
    assert all_e.shape == ref.shape
    print(name, 'max |emb - oracle|', float(np.abs(all_e - ref).max()))
    np.testing.assert_allclose(all_e, ref, rtol=TOL, atol=TOL)
    rng = np.random.default_rng(1)
    for count in COUNTS:
        idx = rng.integers(0, G, size=count)             # permuted, with repeats
        idx[:min(count, 4)] = rng.permutation(4)[:min(count, 4)]   # counts 1, 8, 9, Padding dim
        e = model.embed(store, idx).cpu().numpy()
        assert e.shape == (count, ref.shape[1])
        np.testing.assert_allclose(e, ref[idx], rtol=TOL, atol=TOL)
        assert np.array_equal(e, all_e[idx])             # a graph's row is position-independent


@pytest.mark.parametrize('name', ['default', 'attention', 'pad30_nmax32'])
def test_embeddings_ignore_dropout(gpu, name):
    import torch
    prob, model, store, _ = _embed_case(name, gpu)
    dropped = gpu_model(prob, gpu, dropout=0.1)
    assert dropped.sg.keep_prob < 1.0 and model.sg.keep_prob == 1.0
    idx = np.random.default_rng(2).integers(0, len(store), size=65)
    assert torch.equal(dropped.embed(store, idx), model.embed(store, idx))


def test_embed_status_and_zero_rows(gpu):
    """Ids outside the store and node counts outside [1, Padding dim] are reported in the
    device status and give zero rows; the other rows are unaffected."""
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import GraphStore
    prob, model, store, ref = _embed_case('pad30_nmax32', gpu)
    E, dev = model.embed_dim, store.to_device(gpu)

    def run(dev, idx):
        idx_t = torch.as_tensor(np.asarray(idx), dtype=torch.int32, device=gpu)
        out = torch.full((len(idx), E), 7.0, dtype=torch.float32, device=gpu)
        status = torch.zeros(1, dtype=torch.int32, device=gpu)
        _lib.embed(model.sg, dev, store.n_max, idx_t, len(idx), model.params, out, status)
        return out.cpu().numpy(), int(status.item())

    good, st = run(dev, [0, 1, 2, 3, 4])
    assert st == 0
    np.testing.assert_allclose(good, ref[:5], rtol=TOL, atol=TOL)
    out, st = run(dev, [0, 10_000, 2, -1, 4])            # ids outside the store
    assert st == _lib.SG_ERR_ARG
    assert not out[1].any() and not out[3].any()
    assert np.array_equal(out[[0, 2, 4]], good[[0, 2, 4]])
    out, st = run(dev, [10_000, -5])                     # both sides of a wavefront
    assert st == _lib.SG_ERR_ARG and not out.any()
    # a graph of 31 nodes fits the capacity-32 store but not Padding(30) (A9); n = 0
    big = sized_problem([31, 5, 6], dict(dropout=0.0), n_max=30, seed=11)
    bstore = GraphStore(big.mgs, 32, big.d_in)
    with pytest.raises(_lib.SiameseHipError, match='max_in_dims'):
        model.embed(bstore)                              # the host check of every store
    adj, types, n = bstore.to_device(gpu)
    ok_rows, st = run((adj, types, n), [1, 2])
    assert st == 0
    out, st = run((adj, types, n), [0, 1, 2])
    assert st == _lib.SG_ERR_SHAPE and not out[0].any()
    assert np.array_equal(out[1:], ok_rows)
    n0 = n.clone()
    n0[2] = 0
    out, st = run((adj, types, n0), [1, 2])
    assert st == _lib.SG_ERR_SHAPE and not out[1].any()
    assert np.array_equal(out[0], ok_rows[0])


def test_embed_rejects_web_models_and_wrong_store(gpu):
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import GraphStore
    prob, model, store, _ = _embed_case('default', gpu)
    with pytest.raises(_lib.SiameseHipError, match='n_max'):
        model.embed(GraphStore(prob.mgs, 12, prob.d_in))
    web = sized_problem([5, 40, 12], dict(dropout=0.0), n_max=64, seed=2)
    wm = gpu_model(web, gpu)
    assert wm.is_web
    with pytest.raises(_lib.SiameseHipError):
        wm.embed(GraphStore(web.mgs, 64, web.d_in))
    with pytest.raises(_lib.SiameseHipError):
        wm.score_grid(np.zeros((1, 64), np.float32), np.zeros((1, 64), np.float32))


# ---- score grid -------------------------------------------------------------------------
GRID_SHAPES = ((1, 1), (5, 37), (17, 64), (3, 1000))
SENTINEL = -7.25


def _grid_problem(D, K, ntn_mode='reference', inneract='relu', bias=True, **flags):
    ov = ntn_stack(D, K, inneract, bias, dropout=0.0, ntn_mode=ntn_mode, **flags)
    return sized_problem(_node_counts(D, extra=8, seed=D + K), ov, n_max=D, seed=100 + D + K)


def _rows(emb, idx):
    import torch
    return emb[torch.as_tensor(np.asarray(idx), dtype=torch.long, device=emb.device)]


def _grid(model, eq, edb, final, pad):
    """sg_score_grid into a sentinel-filled buffer of row stride n + pad."""
    import torch
    from graphembedding_amd import _lib
    m, n = int(eq.shape[0]), int(edb.shape[0])
    ws = torch.empty(_lib.score_grid_workspace_bytes(model.sg, m) // 4 + 1, dtype=torch.float32,
                     device=eq.device)
    out = torch.full((m, n + pad), SENTINEL, dtype=torch.float32, device=eq.device)
    _lib.score_grid(model.sg, eq.contiguous(), edb.contiguous(), m, n, model.params, final, out,
                    n + pad, ws)
    out = out.cpu().numpy()
    assert np.all(out[:, n:] == SENTINEL), 'padding columns of out were written'
    return out[:, :n]


def _check_grid(gpu, prob):
    """Every GRID_SHAPE: sg_score_grid (pre-activation) vs sg_forward of the same
    keep_prob = 1 model over the m·n pair list, and vs O.forward at dropout 0."""
    from graphembedding_amd.packer import pack_device
    model = gpu_model(prob, gpu)
    assert model.sg.keep_prob == 1.0
    store = _store(prob, model)
    G = len(store)
    emb = model.embed(store)
    gs = oracle_graphs(prob)
    spec = prob.oracle_spec()
    flat = prob.params.astype(np.float64)
    rng = np.random.default_rng(7)
    worst = 0.0
    for m, n in GRID_SHAPES:
        qi, di = rng.integers(0, G, size=m), rng.integers(0, G, size=n)
        pad = 0 if n % 16 == 0 else 3                    # ld_out == n and ld_out > n
        got = _grid(model, _rows(emb, qi), _rows(emb, di), False, pad)
        pairs = np.stack([np.repeat(qi, n), np.tile(di, m)], axis=1).astype(np.int32)
        recs, status = pack_device(store, pairs, None, device=gpu, dtype=model.record_dtype)
        batch = model.batch_from_records(recs, m * n, np.zeros(m * n, np.float32))
        fwd = model.pred_sim_without_act(batch, seed=0).cpu().numpy().reshape(m, n)
        assert int(status.item()) == 0
        ref = O.forward(spec, flat, [gs[i] for i in pairs[:, 0]], [gs[j] for j in pairs[:, 1]],
                        0).reshape(m, n)
        worst = max(worst, float(np.abs(got - fwd).max()), float(np.abs(got - ref).max()))
        np.testing.assert_allclose(got, fwd, rtol=TOL, atol=TOL)
        np.testing.assert_allclose(got, ref, rtol=TOL, atol=TOL)
    print('grid max abs deviation', worst, 'kernel path', model.kernel_path)
    return model


@pytest.mark.parametrize('ntn_mode', ['reference', 'intended'])
@pytest.mark.parametrize('K', [1, 10, 16])
@pytest.mark.parametrize('D', [10, 11, 16, 31])
def test_score_grid_matches_forward_and_oracle(gpu, D, K, ntn_mode):
    _check_grid(gpu, _grid_problem(D, K, ntn_mode))


@pytest.mark.parametrize('ntn_mode', ['reference', 'intended'])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('inneract', ['relu', 'sigmoid'])
def test_score_grid_inner_activation_and_bias(gpu, inneract, bias, ntn_mode):
    """K = 10 of 16 columns: sigmoid(0) = 0.5 of the six padded columns must not count."""
    _check_grid(gpu, _grid_problem(10, 10, ntn_mode, inneract, bias))


@pytest.mark.parametrize('inneract', ['identity', 'tanh'])
def test_score_grid_other_inner_activations(gpu, inneract):
    _check_grid(gpu, _grid_problem(10, 10, 'reference', inneract, True))


@pytest.mark.parametrize('final', ['gaussian', 'identity', 'relu', 'sigmoid', 'tanh'])
def test_score_grid_final_activation(gpu, final):
    """apply_final = 1 against apply_final_act_np of the raw scores, every sg_final."""
    flags = dict(final_act='sim_kernel', sim_kernel='gaussian') if final == 'gaussian' else \
        dict(final_act=final)
    prob = _grid_problem(10, 10, **flags)
    model = gpu_model(prob, gpu)
    store = _store(prob, model)
    emb = model.embed(store)
    rng = np.random.default_rng(9)
    qi, di = rng.integers(0, len(store), size=5), rng.integers(0, len(store), size=37)
    raw = _grid(model, _rows(emb, qi), _rows(emb, di), False, 3)
    act = _grid(model, _rows(emb, qi), _rows(emb, di), True, 3)
    # element by element: the reference's sigmoid_np takes scalars (math.exp)
    want = np.array([[float(model.apply_final_act_np(float(x))) for x in row] for row in raw])
    np.testing.assert_allclose(act, want, rtol=TOL, atol=TOL)
    if final in ('gaussian', 'sigmoid', 'tanh'):         # (relu keeps these positive scores)
        assert not np.array_equal(act, raw)
    # the model-level wrapper: final=True is the default
    assert np.array_equal(model.score_grid(_rows(emb, qi), _rows(emb, di)).cpu().numpy(), act)
    assert np.array_equal(model.score_grid(_rows(emb, qi), _rows(emb, di), final=False).cpu().numpy(), raw)


# ---- top-k ------------------------------------------------------------------------------
def _topk_rows(n, seed):
    """Rows with runs of equal values, ±inf, ±0, NaNs, and an all-NaN row."""
    rng = np.random.default_rng(seed)
    v = np.round(rng.standard_normal((7, n)) * 2).astype(np.float32) / 2   # many ties
    v[1] = rng.standard_normal(n).astype(np.float32)                     # (almost) no ties
    v[2] = 1.5                                                           # one run
    for r in (3, 4):
        k = max(1, n // 5)
        v[r, rng.integers(0, n, size=k)] = np.inf
        v[r, rng.integers(0, n, size=k)] = -np.inf
        v[r, rng.integers(0, n, size=k)] = np.nan
        v[r, rng.integers(0, n, size=k)] = -0.0
    v[4, rng.integers(0, n, size=max(1, n // 2))] = np.nan
    v[5] = np.nan                                                        # all NaN
    v[6, ::2] = np.nan
    return v


def _topk_ref(v, k, largest):
    idx = np.empty((v.shape[0], k), np.int64)
    for r, row in enumerate(v):
        nan = np.isnan(row)
        key = np.where(nan, 0.0, -row if largest else row).astype(np.float64)
        idx[r] = np.lexsort((np.arange(row.size), key, nan))[:k]   # NaN last, value, column
    return idx


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_topk_rows_matches_lexsort(gpu, n):
    import torch
    from graphembedding_amd import _lib
    v = _topk_rows(n, seed=n)
    rows, ld = v.shape[0], n + 3
    buf = np.full((rows, ld), 123.0, np.float32)
    buf[:, :n] = v
    dev = torch.from_numpy(buf).to(gpu)
    for k in sorted({1, min(10, n), min(n, 64)}):
        for largest in (True, False):
            idx = torch.full((rows, k), -1, dtype=torch.int32, device=gpu)
            val = torch.zeros((rows, k), dtype=torch.float32, device=gpu)
            _lib.topk_rows(dev, rows, n, ld, k, largest, idx, val)
            want = _topk_ref(v, k, largest)
            got = idx.cpu().numpy()
            assert np.array_equal(got, want), (n, k, largest)
            assert np.array_equal(val.cpu().numpy().view(np.uint32),
                                  np.take_along_axis(v, want, axis=1).view(np.uint32))
            idx2 = torch.full((rows, k), -1, dtype=torch.int32, device=gpu)
            _lib.topk_rows(dev, rows, n, ld, k, largest, idx2, None)    # val_out = NULL
            assert torch.equal(idx2, idx)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), buf.view(np.uint32))   # read only


# ---- end to end -------------------------------------------------------------------------
def test_train_test_embed_path(gpu):
    """train.test(test_path='embed') fills the AIDS80nef-shaped test matrix of test_gpu_e2e
    within TOL of the 'pairs' path at dropout 0, and does not depend on flags.dropout."""
    from graphembedding_amd.config import Flags
    from graphembedding_amd.model_mse import create_model
    from graphembedding_amd.train import main, test
    f = Flags(dataset='syn_aids80nef', iters=2, n_max=10, node_feat_order='sorted', dropout=0.0)
    assert f.test_path == 'pairs'
    _, (sim_pairs, _, _), (data, dc, model) = main(f, device=gpu, return_objects=True)
    fe = f.copy(test_path='embed')
    sim_embed, time_mat, _ = test(data, dc, model, fe, None, verbose=False)
    assert sim_embed.shape == sim_pairs.shape == (10, 70)
    print('embed vs pairs max abs', float(np.abs(sim_embed - sim_pairs).max()))
    np.testing.assert_allclose(sim_embed, sim_pairs, rtol=TOL, atol=TOL)
    assert time_mat.shape == (10, 70) and len(np.unique(time_mat)) == 1 and time_mat[0, 0] > 0
    # same parameters, dropout 0.1: 'embed' is inference mode, bit for bit the same
    f1 = fe.copy(dropout=0.1)
    m1 = create_model(f1.model, data.input_dim(), f1, device=gpu, n_max=model.n_max,
                      params=model.flat_params())
    sim1, _, _ = test(data, dc, m1, f1, None, verbose=False)
    assert np.array_equal(sim1, sim_embed)
    # compat_diag handling is the 'pairs' path's
    diag, _, _ = test(data, dc, model, fe.copy(test_matrix='compat_diag'), None, verbose=False)
    expect = np.zeros_like(sim_embed)
    for i in range(10):
        expect[i][i] = sim_embed[i][69]
    assert np.array_equal(diag, expect)
    with pytest.raises(RuntimeError, match='per_pair'):
        test(data, dc, model, fe.copy(test_time='per_pair'), None, verbose=False)
    with pytest.raises(RuntimeError, match='test_path'):
        test(data, dc, model, f.copy(test_path='nope'), None, verbose=False)


def test_embedding_index(gpu):
    import torch
    from graphembedding_amd.retrieval import EmbeddingIndex
    prob, model, store, ref = _embed_case('default', gpu)
    db, queries = prob.mgs[:15], prob.mgs[12:]
    index = EmbeddingIndex(model, db)
    assert index.n == 15 and tuple(index.embeddings.shape) == (15, 10)
    np.testing.assert_allclose(index.embeddings.cpu().numpy(), ref[:15], rtol=TOL, atol=TOL)
    s = index.scores(queries)
    assert tuple(s.shape) == (len(queries), 15)
    assert torch.all((s > 0) & (s <= 1))                 # gaussian similarities
    idx, sims = index.topk(queries, 4)
    idx2, sims2 = model.topk(s, 4)
    assert torch.equal(idx, idx2) and torch.equal(sims, sims2)
    assert torch.equal(sims, torch.gather(s, 1, idx.long()))
    assert torch.all(sims[:, :-1] >= sims[:, 1:])
    # a query that is in the index scores itself like any pair of the pairwise path
    raw = index.scores(queries, final=False).cpu().numpy()
    spec, flat, gs = prob.oracle_spec(), prob.params.astype(np.float64), oracle_graphs(prob)
    want = O.forward(spec, flat, [gs[12 + i] for i in range(len(queries)) for _ in range(15)],
                     [gs[j] for _ in range(len(queries)) for j in range(15)], 0)
    np.testing.assert_allclose(raw.reshape(-1), want, rtol=TOL, atol=TOL)
