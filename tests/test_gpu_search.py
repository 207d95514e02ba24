"""Embed-once search on the GPU (include/siamese_search.h): sg_search_topk against
sg_score_grid + sg_topk_rows bit for bit (indices, and values as int32) over every path
of the segment split, against numpy lexsort on ties, NaNs and signed zeros, against the
oracle's scores independently of the grid kernel, and through EmbeddingIndex.search."""
import numpy as np
import pytest

from _embed_fixtures import gpu_model, oracle_graphs, sized_problem
from oracle import siamese_oracle as O
from test_gpu_embed import _embed_case, _grid_problem, _oracle_embeddings, _topk_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's per-pair parity bar (test_gpu_parity.TOL)
_MODELS = {}


def _model(gpu, D=10, K=10, **kw):
    """A model over the default stack with an NTN head of width D and K feature maps."""
    key = (D, K) + tuple(sorted(kw.items()))
    if key not in _MODELS:
        _MODELS[key] = gpu_model(_grid_problem(D, K, **kw), gpu)
    return _MODELS[key]


def _synthetic(gpu, rows, D, seed):
    """Embeddings as the padded node features give them: uniform in [0, 1)."""
    import torch
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(0, 1, size=(rows, D)).astype(np.float32)).to(gpu)


def _two_call(model, eq, edb, k, largest, final):
    s = model.score_grid(eq, edb, final=final)
    idx, val = model.topk(s, k, largest=largest)
    return idx, val, s


def _same(got, want):
    import torch
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32),
                                                        want[1].view(torch.int32))


def _check(gpu, D=10, K=10, m=5, n=200, ks=(5,), largest=(True,), final=(True,), segs=(64,)):
    model = _model(gpu, D, K)
    eq, edb = _synthetic(gpu, m, D, 1000 + m), _synthetic(gpu, n, D, 2000 + n)
    for fin in final:
        for lg in largest:
            for k in ks:
                want = _two_call(model, eq, edb, k, lg, fin)
                for seg in segs:
                    got = model.search(eq, edb, k, largest=lg, final=fin, seg_cols=seg)
                    assert got[0].dtype == want[0].dtype and got[0].shape == (m, k)
                    assert _same(got, want), (D, K, m, n, k, lg, fin, seg)


# ---- 1. equals the two-call path, bitwise: a base case, then one axis at a time ---------
@pytest.mark.parametrize('D,K', [(10, 10), (11, 1), (16, 16), (31, 16)])
def test_search_equals_two_calls_head_shapes(gpu, D, K):
    """MFMA k-steps NS = 3, 3, 5, 8; four segments, the last with 8 live columns."""
    _check(gpu, D=D, K=K, segs=(0, 64))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 200, 1000])
def test_search_equals_two_calls_sizes(gpu, n):
    """Every k and seg_cols at every n, for one query and for five (two query chunks at
    n = 1000): n = 65 is two segments with one column in the second, n = 200 at seg 64 four
    with fewer than k candidates in the last."""
    ks = sorted({1, min(5, n), min(n, 64)})
    for m in (1, 5):
        _check(gpu, m=m, n=n, ks=ks, segs=(0, 64, 128))


@pytest.mark.parametrize('m,n,k', [(130, 4160, 5), (700, 8192, 64)])
def test_search_equals_two_calls_query_chunks(gpu, m, n, k):
    """More workgroups than the device asks for, so a wavefront walks several queries: at
    seg 64, 65 segments x 17 chunks of 8 queries, and 128 segments x 18 chunks of 40 (the
    most whose k = 64 lists fit a workgroup's LDS).  The library's own segments (1024
    columns here) give chunks of 4."""
    _check(gpu, m=m, n=n, ks=(k,), segs=(64, 0))


@pytest.mark.parametrize('largest', [False, True])
@pytest.mark.parametrize('final', [False, True])
def test_search_equals_two_calls_order_and_final(gpu, largest, final):
    _check(gpu, ks=(1, 5, 64), largest=(largest,), final=(final,), segs=(0, 64, 128))


@pytest.mark.parametrize('kw', [dict(ntn_mode='intended'), dict(inneract='sigmoid', bias=False),
                                dict(inneract='tanh'), dict(final_act='sigmoid')],
                         ids=['intended', 'sigmoid_nobias', 'tanh', 'final_sigmoid'])
def test_search_equals_two_calls_head_options(gpu, kw):
    model = _model(gpu, **kw)
    eq, edb = _synthetic(gpu, 5, 10, 3), _synthetic(gpu, 200, 10, 4)
    for final in (False, True):
        want = _two_call(model, eq, edb, 5, True, final)
        assert _same(model.search(eq, edb, 5, final=final, seg_cols=64), want)


# ---- 2. seg_cols does not change the result --------------------------------------------
def test_search_is_independent_of_seg_cols(gpu):
    model = _model(gpu)
    eq, edb = _synthetic(gpu, 9, 10, 5), _synthetic(gpu, 1000, 10, 6)
    for k in (10, 64):
        outs = [model.search(eq, edb, k, seg_cols=seg) for seg in (64, 256, 1024, 0)]
        for o in outs[1:]:
            assert _same(o, outs[0]), k
        assert _same(outs[0], _two_call(model, eq, edb, k, True, True))


# ---- 3. ties and special values ----------------------------------------------------------
def _check_order(model, eq, edb, k, final, segs=(64, 0)):
    """Both orders: search == two calls bitwise, and the indices are the lexsort of the
    two-call scores (NaN last, value, column)."""
    s = model.score_grid(eq, edb, final=final)
    v = s.cpu().numpy()
    for largest in (True, False):
        want = model.topk(s, k, largest=largest)
        ref = _topk_ref(v, k, largest)
        assert np.array_equal(want[0].cpu().numpy(), ref)
        for seg in segs:
            got = model.search(eq, edb, k, largest=largest, final=final, seg_cols=seg)
            assert _same(got, want), (largest, seg)
            assert np.array_equal(got[0].cpu().numpy(), ref)
            assert np.array_equal(got[1].cpu().numpy().view(np.uint32),
                                  np.take_along_axis(v, ref, axis=1).view(np.uint32))
    return v


def test_search_ties_cross_segments(gpu):
    """Database row j = row j mod 7, n = 130, k = 64 at seg 64: every score repeats 18 or 19
    times over three segments and a tie resolves to the smaller column."""
    model = _model(gpu)
    eq = _synthetic(gpu, 5, 10, 7)
    edb = _synthetic(gpu, 7, 10, 8)[np.arange(130) % 7]
    for final in (True, False):
        v = _check_order(model, eq, edb, 64, final)
        assert np.array_equal(v[:, :7], v[:, 7:14])


def test_search_nan_rows(gpu):
    """A NaN database row ranks last in both orders; an all-NaN query row returns columns
    0 .. k - 1.  (The identity inner activation: relu's x > 0 ? x : 0 maps NaN to 0.)"""
    model = _model(gpu, inneract='identity')
    eq, edb = _synthetic(gpu, 3, 10, 9), _synthetic(gpu, 130, 10, 10)
    edb[3] = float('nan')
    edb[100] = float('nan')
    eq[1] = float('nan')
    for k in (5, 64):
        v = _check_order(model, eq, edb, k, False)
    assert np.isnan(v[1]).all() and np.isnan(v[0, [3, 100]]).all()
    assert np.isnan(v[0]).sum() == 2
    idx, _ = model.search(eq, edb, 64, final=False, seg_cols=64)
    assert np.array_equal(idx[1].cpu().numpy(), np.arange(64))
    idx, _ = model.search(eq[:1], edb[:66], 64, largest=False, final=False, seg_cols=64)
    assert 3 not in idx.cpu().numpy()          # 66 columns, one NaN: it is rank 66
    idx, _ = model.search(eq[:1], edb[:64], 64, largest=False, final=False, seg_cols=64)
    assert idx[0, -1].item() == 3              # k = n: it comes last


def test_search_zero_ties(gpu):
    """relu as the final activation over negative pre-activations (every U_k negative, so
    s = ΣU · Σ relu(m_k) <= 0): the whole row ties at 0 and the result is columns
    0 .. k - 1; without the final activation the scores mix -0 (zero embeddings) with
    negative numbers, and -0 ranks with +0."""
    prob = _grid_problem(10, 10, final_act='relu')
    K = 10
    params = prob.params.copy()
    params[-2 * K:-K] = -np.abs(params[-2 * K:-K]) - np.float32(0.01)   # U; then the bias
    params[-K:] = 0
    from graphembedding_amd.model_mse import SiameseGCNTNMSE
    model = SiameseGCNTNMSE(prob.d_in, prob.flags, device=gpu, n_max=prob.n_max, params=params)
    eq, edb = _synthetic(gpu, 3, 10, 11), _synthetic(gpu, 130, 10, 12)
    eq[2] = 0
    edb[5] = 0
    edb[77] = 0
    raw = _check_order(model, eq, edb, 64, False)
    assert (raw <= 0).all() and (raw < 0).any()
    assert np.signbit(raw[2, [5, 77]]).all() and (raw[2, [5, 77]] == 0).all()   # -0
    act = _check_order(model, eq, edb, 64, True)
    assert not act.any() and not np.signbit(act).any()
    idx, val = model.search(eq, edb, 64, seg_cols=64)
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(64), (3, 1)))
    assert not val.cpu().numpy().any()


# ---- 4. against the oracle, independently of the grid kernel ----------------------------
def test_search_against_oracle(gpu):
    """Default stack, 40 graphs embedded by the oracle at dropout 0, every graph a query,
    k = 5, pre-activation scores."""
    rng = np.random.default_rng(21)
    prob = sized_problem([int(x) for x in rng.integers(1, 11, size=40)], dict(dropout=0.0),
                         n_max=10, seed=23)
    model = gpu_model(prob, gpu)
    emb = _oracle_embeddings(prob).astype(np.float32)
    G, k = 40, 5
    gs, spec, flat = oracle_graphs(prob), prob.oracle_spec(), prob.params.astype(np.float64)
    want = O.forward(spec, flat, [gs[i] for i in range(G) for _ in range(G)],
                     [gs[j] for _ in range(G) for j in range(G)], 0).reshape(G, G)
    for largest in (True, False):
        idx, val = model.search(emb, emb, k, largest=largest, final=False)
        idx, val = idx.cpu().numpy().astype(np.int64), val.cpu().numpy().astype(np.float64)
        at = np.take_along_axis(want, idx, axis=1)
        print('largest', largest, 'max |value - oracle|', float(np.abs(val - at).max()))
        assert np.abs(val - at).max() <= TOL
        assert all(len(set(r)) == k for r in idx)
        # the k-th returned column against the oracle's (k + 1)-th best: one parity bar
        # on each of the two scores
        ranked = np.sort(want, axis=1)
        if largest:
            assert np.all(at[:, k - 1] >= ranked[:, ::-1][:, k] - 2 * TOL)
        else:
            assert np.all(at[:, k - 1] <= ranked[:, k] + 2 * TOL)


# ---- 5. end to end ----------------------------------------------------------------------
def test_embedding_index_search(gpu):
    import torch
    from graphembedding_amd.retrieval import EmbeddingIndex
    prob, model, store, ref = _embed_case('default', gpu)
    db, queries = prob.mgs[:15], prob.mgs[12:]
    index = EmbeddingIndex(model, db)
    for k in (1, 4, 15):
        for largest in (True, False):
            idx, sims = index.topk(queries, k, largest=largest)
            idx2, sims2 = index.search(queries, k, largest=largest)
            assert torch.equal(idx, idx2) and torch.equal(sims.view(torch.int32),
                                                          sims2.view(torch.int32))


# ---- 6. replay, streams, what is written ------------------------------------------------
def test_search_replay_stream_and_bounds(gpu):
    import torch
    from graphembedding_amd import _lib
    model = _model(gpu)
    m, n, k = 6, 300, 7
    eq, edb = _synthetic(gpu, m, 10, 13), _synthetic(gpu, n, 10, 14)
    want = _two_call(model, eq, edb, k, True, True)
    for seg in (0, 64):
        ws = torch.empty(_lib.search_workspace_bytes(model.sg, m, n, k, seg) // 4 + 1,
                         dtype=torch.float32, device=gpu)
        pad = 16
        ibuf = torch.full((m * k + 2 * pad,), -77, dtype=torch.int32, device=gpu)
        vbuf = torch.full((m * k + 2 * pad,), -7.25, dtype=torch.float32, device=gpu)
        idx, val = ibuf[pad:pad + m * k], vbuf[pad:pad + m * k]
        side = torch.cuda.Stream(device=gpu)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _lib.search_topk(model.sg, eq, edb, m, n, model.params, True, k, True, seg, idx, val,
                             ws, stream=side.cuda_stream)
        side.synchronize()
        first = (idx.clone().view(m, k), val.clone().view(m, k))
        assert _same(first, want), seg
        for buf, fill in ((ibuf, -77), (vbuf, -7.25)):
            assert torch.all(buf[:pad] == fill) and torch.all(buf[pad + m * k:] == fill)
        # again into the same buffers, on the current stream
        _lib.search_topk(model.sg, eq, edb, m, n, model.params, True, k, True, seg, idx, val, ws)
        torch.cuda.synchronize()
        assert _same((idx.view(m, k), val.view(m, k)), first), seg
        # val_out = NULL
        idx2 = torch.full((m, k), -1, dtype=torch.int32, device=gpu)
        _lib.search_topk(model.sg, eq, edb, m, n, model.params, True, k, True, seg, idx2, None,
                         ws)
        assert torch.equal(idx2, first[0])
        for buf, fill in ((ibuf, -77), (vbuf, -7.25)):
            assert torch.all(buf[:pad] == fill) and torch.all(buf[pad + m * k:] == fill)
