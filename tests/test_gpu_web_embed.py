"""Embed-once retrieval for graph-store (Web) models on the GPU
(include/siamese_web_embed.h): embeddings from a CSR store against the oracle's node stack,
the large-D NTN score grid against sg_web_forward of a dropout-0 model and against the
oracle's pair forward, and the wiring through EmbeddingIndex and train.test.
Tolerance: the project's per-pair 1e-4 (test_gpu_parity.TOL), rtol = atol."""
import numpy as np
import pytest

from _embed_fixtures import gpu_model, ntn_stack, oracle_graphs, sized_problem
from oracle import siamese_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -7.25
COUNTS = (1, 7, 64, 300)   # one graph, an odd count, many units, more entries than graphs


def _counts(first, D, extra, seed):
    rng = np.random.default_rng(seed)
    return list(first) + [int(x) for x in rng.integers(1, D + 1, size=extra)]


def _pad(D, value):
    return 'Padding:max_in_dims={},padding_value={}'.format(D, value)


# name: (node counts, D, flag overrides, node types)
EMBED_CASES = {
    'd64': (_counts([1, 15, 16, 17, 63, 64], 64, 10, 3), 64, ntn_stack(64, 10), 29),
    'd50': (_counts([1, 16, 33, 50], 50, 6, 4), 50, ntn_stack(50, 10), 29),   # D % 4 != 0
    'd512_k16': ([1, 496, 511, 512], 512, ntn_stack(512, 16), 60),
    'd64_pad1': (_counts([1, 15, 16, 17, 63, 64], 64, 10, 3), 64,
                 ntn_stack(64, 10, layer_3=_pad(64, 1)), 29),
}


def _alive(prob):
    """The Dense layer's bias at +0.5: with the fixtures' small random parameters its relu is
    dead for most of these graphs and every embedding is zero, so the scores would test the
    head's bias term only.  The problem's parameters are what both sides read."""
    from graphembedding_amd.model_mse import param_shapes
    off = 0
    for li, name, shape in param_shapes(prob.layers, prob.d_in):
        n = int(np.prod(shape))
        if li == 2 and name == 'bias':
            prob.params[off:off + n] = 0.5
        off += n
    return prob


def _live_fraction(prob, emb):
    """Fraction of the graphs' own node columns that are non-zero in emb [G'][D], the
    embeddings of the problem's first G' graphs."""
    ns = [m.num_nodes() for m in prob.mgs[:emb.shape[0]]]
    return sum(int((emb[i, :n] != 0).sum()) for i, n in enumerate(ns)) / float(sum(ns))


def _oracle_embeddings(prob):
    """O._node_forward of every graph at dropout 0, padded to D: [G][D] float64."""
    spec = prob.oracle_spec()
    assert spec.keep_prob == 1.0
    P = O.unflatten(spec, prob.params.astype(np.float64))
    return np.stack([np.asarray(O._node_forward(spec, P, g, 0, 0, 0)[0]).reshape(-1)
                     for g in oracle_graphs(prob)])


def _csr(prob, model):
    from graphembedding_amd.web import CsrStore
    return CsrStore(prob.mgs, prob.d_in, model.n_max)


_CACHE = {}


def _case(name, gpu):
    """Problem, model, CSR store and oracle embeddings of a case: built once, read only."""
    if name not in _CACHE:
        counts, D, ov, n_types = EMBED_CASES[name]
        prob = _alive(sized_problem(counts, dict(ov, dropout=0.0), n_max=D, seed=11,
                                    n_types=n_types))
        model = gpu_model(prob, gpu)
        assert model.is_web and model.web_embed_dim == D
        _CACHE[name] = (prob, model, _csr(prob, model), _oracle_embeddings(prob))
    return _CACHE[name]


def _raw(emb, ld):
    """The [count][ld] buffer behind the [count][D] view web_embed returns."""
    import torch
    assert emb.stride(1) == 1 and (emb.shape[0] < 2 or emb.stride(0) == ld)
    return torch.as_strided(emb, (emb.shape[0], ld), (ld, 1), emb.storage_offset())


@pytest.mark.parametrize('name', list(EMBED_CASES))
def test_web_embeddings_match_oracle(gpu, name):
    from graphembedding_amd import _lib
    prob, model, store, ref = _case(name, gpu)
    D = EMBED_CASES[name][1]
    if name == 'd512_k16':
        assert prob.d_in > 48, prob.d_in
    G = len(store)
    ld = _lib.web_embed_ld(model.sg)
    assert ld % 128 == 0 and ld >= D
    all_t = model.web_embed(store)                      # graph_idx = None: every graph
    assert tuple(all_t.shape) == (G, D)
    all_e = all_t.cpu().numpy()
    print(name, 'max |emb - oracle|', float(np.abs(all_e - ref).max()),
          'live node outputs', _live_fraction(prob, ref))
    assert _live_fraction(prob, ref) > 0.5               # not the all-zero embedding
    np.testing.assert_allclose(all_e, ref, rtol=TOL, atol=TOL)
    raw = _raw(all_t, ld).cpu().numpy()
    assert np.array_equal(raw[:, :D], all_e) and not raw[:, D:].any()   # columns [D, ld) zero
    if name == 'd64_pad1':
        n0 = int(store.n[0])
        assert np.all(all_e[0, n0:] == 1.0)             # padding_value past the graph's nodes
    rng = np.random.default_rng(1)
    for count in COUNTS:
        idx = rng.integers(0, G, size=count)             # permuted, with repeats
        idx[:min(count, 4)] = rng.permutation(4)[:min(count, 4)]
        e_t = model.web_embed(store, idx)
        e = e_t.cpu().numpy()
        assert e.shape == (count, D)
        np.testing.assert_allclose(e, ref[idx], rtol=TOL, atol=TOL)
        assert np.array_equal(e, all_e[idx])             # a graph's row is position-independent
        assert not _raw(e_t, ld).cpu().numpy()[:, D:].any()


def test_web_embeddings_ignore_dropout(gpu):
    import torch
    prob, model, store, _ = _case('d64', gpu)
    dropped = gpu_model(prob, gpu, dropout=0.1)
    assert dropped.is_web and dropped.sg.keep_prob < 1.0 and model.sg.keep_prob == 1.0
    idx = np.random.default_rng(2).integers(0, len(store), size=65)
    assert torch.equal(dropped.web_embed(store, idx), model.web_embed(store, idx))


def test_web_embed_status_and_zero_rows(gpu):
    """Ids outside the store are reported in the device status and give zero rows; the
    other rows are unaffected; an empty call is fine."""
    import torch
    from graphembedding_amd import _lib
    prob, model, store, ref = _case('d64', gpu)
    ld, dev = _lib.web_embed_ld(model.sg), store.to_device(gpu)

    def run(idx):
        idx_t = torch.as_tensor(np.asarray(idx, np.int64), dtype=torch.int32, device=gpu)
        out = torch.full((max(len(idx), 1), ld), 7.0, dtype=torch.float32, device=gpu)
        status = torch.zeros(1, dtype=torch.int32, device=gpu)
        ws = torch.empty(_lib.web_embed_workspace_bytes(model.sg, len(idx)) // 4 + 1,
                         dtype=torch.float32, device=gpu)
        _lib.web_embed(model.sg, dev, idx_t, len(idx), model.params, out, ws, status)
        return out.cpu().numpy()[:len(idx)], int(status.item())

    good, st = run([0, 1, 2, 3, 4])
    assert st == 0
    np.testing.assert_allclose(good[:, :64], ref[:5], rtol=TOL, atol=TOL)
    out, st = run([0, 10_000, 2, -1, 4])                 # past the store, and negative
    assert st == _lib.SG_ERR_ARG
    assert not out[1].any() and not out[3].any()
    assert np.array_equal(out[[0, 2, 4]], good[[0, 2, 4]])
    out, st = run([len(store), -5])
    assert st == _lib.SG_ERR_ARG and not out.any()
    out, st = run([])
    assert st == 0 and out.shape[0] == 0
    assert tuple(model.web_embed(store, []).shape) == (0, 64)


# ---- score grid -------------------------------------------------------------------------
GRID_SHAPES = ((1, 1), (5, 37), (17, 64), (3, 200))


def _grid_problem(D, K=10, first=None, extra=8, n_types=29, **kw):
    layer3 = kw.pop('layer_3', None)
    bias = kw.pop('bias', True)
    ov = ntn_stack(D, K, 'relu', bias, dropout=0.0, **kw)
    if layer3:
        ov['layer_3'] = layer3
    counts = _counts([1, D] if first is None else first, D, extra, D + K)
    return _alive(sized_problem(counts, ov, n_max=D, seed=100 + D + K, n_types=n_types))


def _grid(model, eq, edb, final, pad):
    """sg_web_score_grid into a sentinel-filled buffer of row stride n + pad; the
    embeddings' own row strides are passed."""
    import torch
    from graphembedding_amd import _lib
    m, n = int(eq.shape[0]), int(edb.shape[0])
    d = model.web_embed_dim
    ws = torch.empty(_lib.web_score_grid_workspace_bytes(model.sg, m) // 4 + 1,
                     dtype=torch.float32, device=eq.device)
    out = torch.full((m, n + pad), SENTINEL, dtype=torch.float32, device=eq.device)
    assert eq.stride(1) == 1 and edb.stride(1) == 1
    _lib.web_score_grid(model.sg, eq, max(d, eq.stride(0)), edb, max(d, edb.stride(0)), m, n,
                        model.params, final, out, n + pad, ws)
    out = out.cpu().numpy()
    assert np.all(out[:, n:] == SENTINEL), 'padding columns of out were written'
    return out[:, :n]


def _check_grid(gpu, prob, shapes):
    """sg_web_score_grid (pre-activation) vs (a) sg_web_forward of the same dropout-0 model
    over the m·n pair list and (b) O.forward; final=True vs apply_final_act_np; strided vs
    contiguous embeddings and two calls bitwise."""
    import torch
    model = gpu_model(prob, gpu)
    assert model.is_web and model.sg.keep_prob == 1.0
    store = _csr(prob, model)
    G = len(store)
    emb = model.web_embed(store)
    D = model.web_embed_dim
    assert _live_fraction(prob, emb.cpu().numpy()) > 0.5               # W and V terms count
    gs = oracle_graphs(prob)
    spec = prob.oracle_spec()
    flat = prob.params.astype(np.float64)
    rng = np.random.default_rng(7)
    for m, n in shapes:
        qi, di = rng.integers(0, G, size=m), rng.integers(0, G, size=n)
        qt = torch.as_tensor(qi, dtype=torch.long, device=gpu)
        dt = torch.as_tensor(di, dtype=torch.long, device=gpu)
        ld = emb.stride(0)
        eq = torch.as_strided(emb, (G, ld), (ld, 1))[qt][:, :D]       # strided rows, ld >= D
        edb = torch.as_strided(emb, (G, ld), (ld, 1))[dt][:, :D]
        assert eq.stride(0) == ld or m == 1
        got = _grid(model, eq, edb, False, 3)                         # ld_out = n + 3
        pairs = np.stack([np.repeat(qi, n), np.tile(di, m)], axis=1).astype(np.int32)
        batch = model.web_batch(store, torch.from_numpy(pairs).to(gpu),
                                np.zeros(m * n, np.float32))
        fwd = model.pred_sim_without_act(batch, seed=0).cpu().numpy().reshape(m, n)
        ref = O.forward(spec, flat, [gs[i] for i in pairs[:, 0]], [gs[j] for j in pairs[:, 1]],
                        0).reshape(m, n)
        print('grid D', D, 'K', model.sg.layers[4].output_dim, (m, n),
              'max |grid - forward|', float(np.abs(got - fwd).max()),
              'max |grid - oracle|', float(np.abs(got - ref).max()),
              'max |forward - oracle|', float(np.abs(fwd - ref).max()))
        np.testing.assert_allclose(got, fwd, rtol=TOL, atol=TOL)
        np.testing.assert_allclose(got, ref, rtol=TOL, atol=TOL)
        # contiguous [.][D] copies (ld = D, any D) and a second call: the same bits
        assert np.array_equal(_grid(model, eq.contiguous(), edb.contiguous(), False, 0), got)
        assert np.array_equal(_grid(model, eq, edb, False, 3), got)
        act = _grid(model, eq, edb, True, 3)
        want = np.array([[float(model.apply_final_act_np(float(x))) for x in row] for row in got])
        np.testing.assert_allclose(act, want, rtol=TOL, atol=TOL)
        assert np.array_equal(model.web_score_grid(eq, edb).cpu().numpy(), act)
        assert np.array_equal(model.web_score_grid(eq, edb, final=False).cpu().numpy(), got)
    return model


def test_web_score_grid_shapes_d64(gpu):
    _check_grid(gpu, _grid_problem(64), GRID_SHAPES)


GRID_CASES = {
    'd50': dict(D=50),
    'd130': dict(D=130),                                   # two 128-column tiles of the embedding
    'd512_k16': dict(D=512, K=16, first=[1, 512, 200, 450], extra=2, n_types=60),
    'k1': dict(D=64, K=1),
    'intended': dict(D=64, ntn_mode='intended'),
    'no_bias': dict(D=64, bias=False),
    'sigmoid_final': dict(D=64, final_act='sigmoid'),
    'pad1': dict(D=64, layer_3=_pad(64, 1)),
}


@pytest.mark.parametrize('name', list(GRID_CASES))
def test_web_score_grid_cases(gpu, name):
    _check_grid(gpu, _grid_problem(**GRID_CASES[name]), ((5, 37),))


# ---- wiring -----------------------------------------------------------------------------
def test_web_embedding_index(gpu):
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.retrieval import EmbeddingIndex
    prob = _alive(sized_problem(_counts([1, 64], 64, 23, 5), ntn_stack(64, 10, dropout=0.0),
                                n_max=64, seed=21))
    model = gpu_model(prob, gpu)
    assert model.is_web
    db, queries = prob.mgs[:20], prob.mgs[20:]
    assert len(queries) == 5
    index = EmbeddingIndex(model, db)
    assert index.n == 20 and tuple(index.embeddings.shape) == (20, 64)
    assert _live_fraction(prob, index.embeddings.cpu().numpy()) > 0.5
    s = index.scores(queries)
    assert tuple(s.shape) == (5, 20)
    from graphembedding_amd.web import CsrStore
    eq = model.web_embed(CsrStore(queries, prob.d_in, model.n_max))
    assert torch.equal(s, model.web_score_grid(eq, index.embeddings))
    sn = s.cpu().numpy()
    for largest in (True, False):
        idx, sims = index.topk(queries, 4, largest=largest)
        want = np.stack([np.lexsort((np.arange(20), -row if largest else row))[:4] for row in sn])
        assert np.array_equal(idx.cpu().numpy(), want)
        assert np.array_equal(sims.cpu().numpy(), np.take_along_axis(sn, want, axis=1))
    with pytest.raises(_lib.SiameseHipError, match='topk'):
        index.search(queries, 4)
    # the web_* methods are for graph-store models only
    small = sized_problem([3, 5, 8], dict(dropout=0.0), n_max=10, seed=2)
    sm = gpu_model(small, gpu)
    assert not sm.is_web
    with pytest.raises(_lib.SiameseHipError):
        sm.web_embed(CsrStore(small.mgs, small.d_in, 10))
    with pytest.raises(_lib.SiameseHipError):
        sm.web_score_grid(np.zeros((1, 10), np.float32), np.zeros((1, 10), np.float32))


def test_train_test_embed_path_web(gpu):
    """train.test(test_path='embed') on a graph-store model fills the AIDS80nef-shaped test
    matrix within TOL of the 'pairs' path at dropout 0."""
    from graphembedding_amd.config import Flags
    from graphembedding_amd.train import main, test
    f = Flags(dataset='syn_aids80nef', iters=2, n_max=64, node_feat_order='sorted', dropout=0.0,
              **ntn_stack(64, 10))
    _, (sim_pairs, _, _), (data, dc, model) = main(f, device=gpu, return_objects=True)
    assert model.is_web
    sim_embed, time_mat, _ = test(data, dc, model, f.copy(test_path='embed'), None, verbose=False)
    assert sim_embed.shape == sim_pairs.shape == (10, 70)
    print('web embed vs pairs max abs', float(np.abs(sim_embed - sim_pairs).max()))
    np.testing.assert_allclose(sim_embed, sim_pairs, rtol=TOL, atol=TOL)
    assert time_mat.shape == (10, 70) and time_mat[0, 0] > 0
