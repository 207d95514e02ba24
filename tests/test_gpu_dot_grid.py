"""The Dot-head score grid and fused search on the GPU (include/siamese_dot_embed.h).

Bitwise contract: with integer-valued embeddings (entries in -8 .. 8, E <= 512: every partial
sum is an integer below 2^24) each MFMA k-step is exact, so the grid must EQUAL numpy's
E_q @ E_db.T.  Position independence, search == score_grid + topk and tie order are bitwise
too.  Parity with the oracle and with the pair path is held to the project's 1e-4 (rtol = atol,
test_gpu_parity.TOL)."""
import numpy as np
import pytest

import _stack_zoo as Z
from _embed_fixtures import gpu_model, oracle_graphs
from oracle import siamese_oracle as O
from test_dot_embed_abi import dot_model

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = -7.25
DOT_NAMES = [n for n in Z.NAMES if Z.ZOO[n]['flags']['layer_{}'.format(
    Z.ZOO[n]['flags']['num_layers'] - 1)] == 'Dot']

# E -> (Padding rows, width): E = rows * width, rows <= 64, width <= 256
E_SHAPES = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 6: (2, 3), 16: (4, 4), 17: (1, 17),
            64: (8, 8), 65: (5, 13), 160: (10, 16), 511: (7, 73), 512: (32, 16)}
GRID_SHAPES = [(1, 1), (1, 2), (5, 63), (4, 64), (7, 65), (130, 129)]

_MODELS = {}


def _sg(E, **flags):
    key = (E, tuple(sorted(flags.items())))
    if key not in _MODELS:
        _MODELS[key] = dot_model(*E_SHAPES[E], **flags)
    return _MODELS[key]


def _grid(gpu, sg, q, db, final, ld_q=None, ld_db=None, pad_out=0):
    """sg_dot_score_grid on host arrays, rows placed at strides ld_q / ld_db in NaN-filled
    buffers (a read past column E would poison the score), out at stride n + pad_out."""
    import torch
    from graphembedding_amd import _lib
    m, n, E = q.shape[0], db.shape[0], q.shape[1]
    ld_q, ld_db = ld_q or E, ld_db or E
    bq = torch.full((m, ld_q), float('nan'), dtype=torch.float32, device=gpu)
    bdb = torch.full((n, ld_db), float('nan'), dtype=torch.float32, device=gpu)
    bq[:, :E] = torch.from_numpy(q).to(gpu)
    bdb[:, :E] = torch.from_numpy(db).to(gpu)
    out = torch.full((m, n + pad_out), SENTINEL, dtype=torch.float32, device=gpu)
    _lib.dot_score_grid(sg, bq, ld_q, bdb, ld_db, m, n, final, out, n + pad_out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ints(rows, E, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(rows, E)).astype(np.float32)


@pytest.mark.parametrize('E', list(E_SHAPES))
def test_integer_grid_equals_numpy(gpu, E):
    sg = _sg(E)
    for m, n in GRID_SHAPES:
        q, db = _ints(m, E, 10 * E + m), _ints(n, E, 10 * E + n + 1)
        want = q.astype(np.float64) @ db.astype(np.float64).T
        assert np.abs(want).max() < 2 ** 24
        got = _grid(gpu, sg, q, db, False, ld_q=E + 3, ld_db=E + 5, pad_out=7)
        assert np.all(got[:, n:] == SENTINEL), ('columns j >= n were written', E, m, n)
        assert np.array_equal(got[:, :n].astype(np.float64), want), (E, m, n)
        if (m, n) == (7, 65):   # contiguous rows give the same bits
            assert np.array_equal(_grid(gpu, sg, q, db, False), got[:, :n])


@pytest.mark.parametrize('E', [5, 16, 65, 511])
def test_score_does_not_depend_on_position(gpu, E):
    sg = _sg(E)
    rng = np.random.default_rng(E)
    q = rng.standard_normal((130, E)).astype(np.float32)
    db = rng.standard_normal((129, E)).astype(np.float32)
    full = _grid(gpu, sg, q, db, False)
    for i in (0, 5, 63, 64, 129):
        assert np.array_equal(_grid(gpu, sg, q[i:i + 1], db, False)[0], full[i]), i
    perm = rng.permutation(129)
    assert np.array_equal(_grid(gpu, sg, q, db[perm], False), full[:, perm])
    # other strides, other launch shape (a 130 x 2 grid holds columns 0 and 1)
    assert np.array_equal(_grid(gpu, sg, q, db, False, ld_q=E + 1, ld_db=2 * E), full)
    assert np.array_equal(_grid(gpu, sg, q, db[:2], False), full[:, :2])


# ---- search ------------------------------------------------------------------------------
def _search_case(gpu, model, q, db, k, largest, final, seg_cols):
    import torch
    tq, tdb = torch.from_numpy(q).to(gpu), torch.from_numpy(db).to(gpu)
    scores = model.score_grid(tq, tdb, final=final)
    want_i, want_v = model.topk(scores, k, largest=largest)
    got_i, got_v = model.search(tq, tdb, k, largest=largest, final=final, seg_cols=seg_cols)
    torch.cuda.synchronize()
    assert torch.equal(got_i, want_i), (k, largest, final, seg_cols)
    assert torch.equal(got_v.view(torch.int32), want_v.view(torch.int32)), (k, largest, final)
    return got_i.cpu().numpy(), scores.cpu().numpy()


def _avg_dot_model(gpu, name='dot_average_tanh_broadcast'):
    return gpu_model(Z.zoo_problem(name, 0.0), gpu)    # E = 5


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_search_equals_grid_plus_topk(gpu, n):
    model = _avg_dot_model(gpu)
    E = model.embed_dim
    rng = np.random.default_rng(n)
    q = rng.standard_normal((130, E)).astype(np.float32)      # m = 130 crosses a query chunk
    db = rng.standard_normal((n, E)).astype(np.float32)
    for k in sorted({1, min(10, n), min(n, 64)}):
        for largest in (True, False):
            for final in (True, False):
                for seg in ((0, 64, 256) if n == 1000 else (0,)):
                    _search_case(gpu, model, q, db, k, largest, final, seg)


def test_search_ties_go_to_the_smaller_column(gpu):
    """Integer embeddings, every database row present four times, the copies 250 columns
    apart: with seg_cols = 64 the copies of a row lie in different segments, so the order of
    equal scores is decided in the running lists and again in the merge."""
    model = _avg_dot_model(gpu)
    E = model.embed_dim
    base = _ints(250, E, 3)
    db = np.concatenate([base] * 4)                            # n = 1000
    q = _ints(130, E, 4)
    for largest in (True, False):
        for seg in (0, 64, 256):
            idx, scores = _search_case(gpu, model, q, db, 64, largest, False, seg)
            for i in (0, 77, 129):
                row = scores[i].astype(np.float64)
                order = np.lexsort((np.arange(1000), -row if largest else row))[:64]
                assert np.array_equal(idx[i], order), (largest, seg, i)
                # every tie group the list holds entirely is in ascending column order
                assert np.all(np.diff(idx[i])[np.diff(row[idx[i]]) == 0] > 0)


# ---- parity with the oracle and with the pair path ---------------------------------------
def pair_batch(model, store, pairs, labels):
    """The pairs as packed records: a Dot model runs the generic kernel, which has no
    store-sourced batches."""
    import torch
    labels = np.ascontiguousarray(labels, np.float32).reshape(-1)
    words = store.pack_host(pairs, labels, dtype=model.record_dtype)
    recs = torch.from_numpy(words.view(np.int32).reshape(-1)).to(model.params.device)
    return model.batch_from_records(recs, len(pairs), labels)


@pytest.mark.parametrize('name', DOT_NAMES)
def test_zoo_dot_grid_matches_oracle_and_pairs(gpu, name):
    import torch
    from graphembedding_amd.packer import GraphStore
    prob = Z.zoo_problem(name, 0.0)
    model = gpu_model(prob, gpu)
    assert model.is_dot and model.kernel_path == 0
    store = GraphStore(prob.mgs, model.n_max, prob.d_in)
    G, m = len(store), 5
    emb = model.embed(store)
    pairs = np.stack([np.repeat(np.arange(m), G - m), np.tile(np.arange(m, G), m)],
                     axis=1).astype(np.int32)
    labels = np.full(len(pairs), 0.5, np.float32)
    gs = oracle_graphs(prob)
    ref = O.fwd_bwd(prob.oracle_spec(), prob.params.astype(np.float64),
                    [gs[i] for i in pairs[:, 0]], [gs[j] for j in pairs[:, 1]],
                    labels.astype(np.float64), 0)
    batch = pair_batch(model, store, pairs, labels)
    s_pair = model.pred_sim_without_act(batch, seed=0).cpu().numpy()
    s_grid = model.score_grid(emb[:m], emb[m:], final=False).cpu().numpy().reshape(-1)
    print('{}: max |grid - oracle| {:.3g}, |grid - pairs| {:.3g} (max |s| {:.3g})'.format(
        name, float(np.abs(s_grid - ref.s).max()), float(np.abs(s_grid - s_pair).max()),
        float(np.abs(ref.s).max())))
    np.testing.assert_allclose(s_grid, ref.s, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(s_grid, s_pair, rtol=TOL, atol=TOL)
    y_grid = model.score_grid(emb[:m], emb[m:], final=True).cpu().numpy().reshape(-1)
    y_ref = np.asarray(model.apply_final_act_np(ref.s), np.float64).reshape(-1)
    np.testing.assert_allclose(y_grid, y_ref, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(y_grid, np.asarray(model.apply_final_act_np(s_pair)).reshape(-1),
                               rtol=TOL, atol=TOL)


# ---- EmbeddingIndex and train.test on a Dot model ----------------------------------------
def test_embedding_index_and_test_embed_path_on_a_dot_model(gpu, monkeypatch):
    import torch
    from graphembedding_amd import data as D
    from graphembedding_amd.config import Flags
    from graphembedding_amd.eval import Eval
    from graphembedding_amd.retrieval import EmbeddingIndex
    from graphembedding_amd.train import main, test
    # 20 train and 6 test graphs of 3 .. 10 nodes
    monkeypatch.setitem(D.SYNTHETIC, 'syn_dot6x20', (20, 6, 3, 10, 6))
    ov = Z.stack(*Z.NARROW, 'Average', 'Dot', final_act='tanh')
    f = Flags(dataset='syn_dot6x20', iters=2, n_max=10, node_feat_order='sorted', **ov)
    _, _, (data, dc, model) = main(f, device=gpu, return_objects=True)
    assert model.is_dot and data.m_n() == (6, 20)
    out = {}
    for path in ('host', 'device'):
        ev = Eval.from_calculator(data, dc, f)
        sim_mat, time_mat, res = test(data, dc, model, f.copy(test_path='embed', eval_path=path),
                                      ev, verbose=False)
        assert sim_mat.shape == (6, 20)
        out[path] = (sim_mat, res)
    assert np.array_equal(out['host'][0], out['device'][0])
    host, dev = out['host'][1], out['device'][1]
    name = f.model
    for sfx in ('_norm', '_nonorm'):
        assert np.array_equal(dev['apk' + sfx][name]['aps'], host['apk' + sfx][name]['aps'])
        assert dev['mrr' + sfx][name] == host['mrr' + sfx][name]
        np.testing.assert_allclose(dev['mse' + sfx][name], host['mse' + sfx][name], rtol=1e-9,
                                   atol=0)
    # the index: scores are the test matrix; nearest == topk == search, bit for bit
    m, n = data.m_n()
    db = [data.get_orig_train_graph(j) for j in range(n)]
    qs = [data.test_data.get_graph(i) for i in range(m)]
    index = EmbeddingIndex(model, db)
    assert np.array_equal(index.scores(qs).cpu().numpy().astype(np.float64), out['host'][0])
    for k in (1, 5, 20):
        ti, tv = index.topk(qs, k)
        for fused in (index.nearest, index.search):
            gi, gv = fused(qs, k)
            assert torch.equal(gi, ti) and torch.equal(gv, tv), k
