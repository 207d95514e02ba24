"""Embed-once search for graph-store (Web) models on the GPU
(include/siamese_web_search.h): sg_web_search_topk against sg_web_score_grid + sg_topk_rows
bit for bit (indices, and values as int32) over every A-operand instantiation, every path of
the segment and query-chunk split and the block-boundary pipeline, against numpy lexsort on
ties, against the float64 head independently of the grid kernel, and through
EmbeddingIndex.nearest.

Inputs are the dense signed embeddings of _embed_fixtures.grid_ref_embeddings (real Web
embeddings are non-negative and mostly zero, and would hide dropped terms) and the models of
GRID_REF_MODELS, as test_gpu_web_grid_shapes.py uses them."""
import numpy as np
import pytest

from _embed_fixtures import (gpu_model, grid_ref_embeddings, grid_ref_problem, ntn_stack,
                             sized_problem)
from test_gpu_web_embed import _alive, _counts
from test_gpu_web_grid_shapes import WIDTH_CASES, WIDTHS, _cus, _dev, _head, _nsmax, _ref

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's per-pair bar for this head: TOL (1 + |score|)


# ---- what the host code of sg_web_search_topk decides from (m, n, k, seg_cols, CUs) --------
# A transcription of web_search_plan (sg_web_search.hip).  It only guards coverage: a case
# asserts that it reaches the configuration it is meant to before it calls the kernel.  It is
# never a reference for a result.
LIST_LDS = 12288


def _plan(m, n, k, seg_cols, cus):
    target = 2 * cus
    max_qc = (m + 3) // 4 if m > 4 else 1
    seg = seg_cols
    if seg == 0:
        seg = 4096
        while seg < 1024 * k:
            seg <<= 1
        while seg > 1024 and -(-n // seg) * max_qc < target:
            seg >>= 1
    if seg > n:
        seg = (n + 63) & ~63
    nseg = -(-n // seg)
    nqc = min(max_qc, -(-target // nseg))
    cap = (LIST_LDS // (12 * k)) & ~3
    qb = max(4, min(cap, (-(-m // nqc) + 3) & ~3))
    nqc = -(-m // qb)
    return dict(seg=seg, nseg=nseg, qb=qb, nqc=nqc, cap=cap, last=m - (nqc - 1) * qb,
                blocks_per_seg=-(-min(seg, n) // 64))


# ---- embeddings, calls ------------------------------------------------------------------------
_EMB = {}


def _emb(gpu, D, m, n):
    """Device tensors of grid_ref_embeddings: built once per shape, read only."""
    key = (D, m, n)
    if key not in _EMB:
        eq, edb = grid_ref_embeddings(D, m, n)
        _EMB[key] = (_dev(eq, gpu), _dev(edb, gpu), eq, edb)
    return _EMB[key]


def _two_call(model, eq, edb, k, largest, final):
    s = model.web_score_grid(eq, edb, final=final)
    idx, val = model.topk(s, k, largest=largest)
    return idx, val, s


def _same(got, want):
    import torch
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32),
                                                        want[1].view(torch.int32))


def _check(gpu, D=64, K=10, bias=True, ntn_mode='reference', m=5, n=200, ks=(5,),
           largest=(True,), final=(True,), segs=(64,)):
    import torch
    model = _head(gpu, D, K, bias, ntn_mode)[0]
    eq, edb = _emb(gpu, D, m, n)[:2]
    for fin in final:
        for lg in largest:
            for k in ks:
                want = _two_call(model, eq, edb, k, lg, fin)
                for seg in segs:
                    got = model.web_search(eq, edb, k, largest=lg, final=fin, seg_cols=seg)
                    assert got[0].dtype == torch.int32 and tuple(got[0].shape) == (m, k)
                    assert _same(got, want), (D, K, m, n, k, lg, fin, seg)


# ---- 1. widths and instantiations --------------------------------------------------------------
CASES_1 = WIDTH_CASES + [(64, 10, True, 'reference'), (512, 16, True, 'reference')]


@pytest.mark.parametrize('D,K,bias,ntn_mode', CASES_1)
def test_web_search_widths_and_instantiations(gpu, D, K, bias, ntn_mode):
    """Every web_search_kernel<NSMAX> and both sides of each boundary; at seg 64 four
    segments, the last with 8 live columns and fewer than k = 64 candidates."""
    if D in WIDTHS:
        assert _nsmax(D) == WIDTHS[D]
    assert _nsmax(64) == (17, 17) and _nsmax(512) == (129, 129)
    _check(gpu, D=D, K=K, bias=bias, ntn_mode=ntn_mode, ks=(1, 5, 64), segs=(0, 64, 128))


# ---- 2. sizes --------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200, 1000])
def test_web_search_sizes(gpu, n):
    """Every k and seg_cols at every n, for one query and for five: n = 65 is two segments
    with one column in the second, n = 1000 at seg 64 sixteen with 40 columns in the last."""
    ks = sorted({1, min(5, n), min(n, 64)})
    for m in (1, 5):
        _check(gpu, m=m, n=n, ks=ks, segs=(0, 64, 128))


# ---- 3. query chunks and the block-boundary pipeline ------------------------------------------
def _odd_walk(cus, k=5, seg=192):
    """The smallest (n, m): a workgroup walks an odd count of more than four queries over the
    three blocks of a 192-column segment, the last segment short."""
    for s in (16, 32, 64, 128, 256, 512, 1024):
        n = seg * s - 7
        for m in range(9, 200, 2):
            p = _plan(m, n, k, seg, cus)
            if p['qb'] > 4 and p['last'] > 4 and p['last'] % 2 == 1:
                return m, n, p
    pytest.fail('no shape walks an odd chunk of more than 4 queries at {} CUs'.format(cus))


@pytest.mark.parametrize('D,K', [(64, 10), (512, 16)])
def test_web_search_odd_chunk_over_blocks(gpu, D, K):
    """More than four queries, an odd count, over three 64-column blocks per workgroup: the
    table pipeline runs through two block boundaries, the buffer and slot parity of a query
    differ from block to block, and the last query of the last block is taken by the tail."""
    cus = _cus(gpu)
    m, n, p = _odd_walk(cus)
    print('D', D, 'm', m, 'n', n, 'CUs', cus, p)
    assert p['seg'] == 192 and p['blocks_per_seg'] == 3 and p['nseg'] > 1
    assert p['qb'] > 4 and p['last'] > 4 and p['last'] % 2 == 1
    _check(gpu, D=D, K=K, m=m, n=n, ks=(5,), segs=(192, 0))
    # one segment of three blocks (the direct write of idx / val), a last chunk of one query
    q = _plan(5, 192 - 7, 5, 192, cus)
    assert q['nseg'] == 1 and q['qb'] == 4 and q['last'] == 1 and q['blocks_per_seg'] == 3
    _check(gpu, D=D, K=K, m=5, n=192 - 7, ks=(5,), segs=(192,))


def _capped(cus, k=64, seg=64):
    for s in (16, 32, 64, 128, 256, 512, 1024):
        n = seg * s
        for m in range(17, 400):
            p = _plan(m, n, k, seg, cus)
            if p['qb'] == p['cap'] and m % p['cap'] != 0 and p['nqc'] > 1:
                return m, n, p
    pytest.fail('no shape reaches the LDS cap of qb at {} CUs'.format(cus))


@pytest.mark.parametrize('D,K', [(64, 10), (512, 16)])
def test_web_search_qb_at_the_lds_cap(gpu, D, K):
    """k = 64: the lists of 16 queries fill the list LDS; m is not a multiple of 16, so the
    last chunk is partial.  At D = 512 this is the largest LDS request, 79872 B."""
    cus = _cus(gpu)
    m, n, p = _capped(cus)
    print('D', D, 'm', m, 'n', n, 'CUs', cus, p)
    assert p['cap'] == 16 and p['qb'] == 16 and m % 16 != 0 and p['last'] < 16
    _check(gpu, D=D, K=K, m=m, n=n, ks=(64,), segs=(64, 0))


# ---- 4. order and final activation; seg_cols does not change the result ------------------------
@pytest.mark.parametrize('largest', [False, True])
@pytest.mark.parametrize('final', [False, True])
def test_web_search_order_and_final(gpu, largest, final):
    _check(gpu, ks=(1, 5, 64), largest=(largest,), final=(final,), segs=(0, 64, 128))


def test_web_search_is_independent_of_seg_cols(gpu):
    model = _head(gpu, 64, 10)[0]
    eq, edb = _emb(gpu, 64, 9, 1000)[:2]
    for k in (10, 64):
        outs = [model.web_search(eq, edb, k, seg_cols=seg) for seg in (64, 256, 1024, 0)]
        for o in outs[1:]:
            assert _same(o, outs[0]), k
        assert _same(outs[0], _two_call(model, eq, edb, k, True, True))


# ---- 5. ties and special values ----------------------------------------------------------------------
def _topk_ref(v, k, largest):
    """numpy lexsort: NaN last, then by value (descending when largest), then by column."""
    out = []
    for row in v:
        nan = np.isnan(row)
        key = np.where(nan, 0.0, -row if largest else row)
        out.append(np.lexsort((np.arange(len(row)), key, nan))[:k])
    return np.stack(out)


def _check_order(model, eq, edb, k, final, segs=(64, 0)):
    """Both orders: search == two calls bitwise, and the indices are the lexsort of the
    two-call scores."""
    s = model.web_score_grid(eq, edb, final=final)
    v = s.cpu().numpy()
    for largest in (True, False):
        want = model.topk(s, k, largest=largest)
        ref = _topk_ref(v, k, largest)
        assert np.array_equal(want[0].cpu().numpy(), ref)
        for seg in segs:
            got = model.web_search(eq, edb, k, largest=largest, final=final, seg_cols=seg)
            assert _same(got, want), (largest, seg)
            assert np.array_equal(got[0].cpu().numpy(), ref)
            assert np.array_equal(got[1].cpu().numpy().view(np.uint32),
                                  np.take_along_axis(v, ref, axis=1).view(np.uint32))
    return v


def test_web_search_ties_cross_segments(gpu):
    """Database row j = row j mod 7, n = 130, k = 64 at seg 64: every score repeats 18 or 19
    times over three segments and a tie resolves to the smaller column."""
    model = _head(gpu, 64, 10)[0]
    eq, edb7 = _emb(gpu, 64, 5, 7)[:2]
    edb = edb7[np.arange(130) % 7]
    for final in (True, False):
        v = _check_order(model, eq, edb, 64, final)
        assert np.array_equal(v[:, :7], v[:, 7:14])


def _ntn_param(prob, name):
    """(offset, size) of a parameter of the problem's NTN layer in prob.params."""
    from graphembedding_amd.model_mse import param_shapes
    off = 0
    for li, pname, shape in param_shapes(prob.layers, prob.d_in):
        size = int(np.prod(shape))
        if prob.layers[li]['kind'] == 'NTN' and pname == name:
            return off, size
        off += size
    raise KeyError(name)


def _edited_model(gpu, prob, params, **flag_overrides):
    from graphembedding_amd.model_mse import SiameseGCNTNMSE
    flags = prob.flags.copy(**flag_overrides) if flag_overrides else prob.flags
    return SiameseGCNTNMSE(prob.d_in, flags, device=gpu, n_max=prob.n_max, params=params)


def test_web_search_zero_ties(gpu):
    """relu as the final activation with every U_k negative: s = ΣU · Σ relu(m_k) <= 0, so
    every score is 0 and the result is columns 0 .. k - 1, in both orders."""
    prob = grid_ref_problem(64, 10)
    off, size = _ntn_param(prob, 'weights_U')
    assert size == 10
    params = prob.params.copy()
    params[off:off + size] = -np.abs(params[off:off + size]) - np.float32(0.01)
    model = _edited_model(gpu, prob, params, final_act='relu')
    assert model.is_web
    eq, edb = _emb(gpu, 64, 3, 130)[:2]
    raw = model.web_score_grid(eq, edb, final=False).cpu().numpy()
    assert (raw <= 0).all() and (raw < 0).any()          # the head is live under the relu
    act = _check_order(model, eq, edb, 64, True)
    assert not act.any()
    for largest in (True, False):
        for seg in (64, 0):
            idx, val = model.web_search(eq, edb, 64, largest=largest, seg_cols=seg)
            assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(64), (3, 1)))
            assert not val.cpu().numpy().any()


def test_web_search_all_nan(gpu):
    """One U_k = NaN in the reference ntn_mode (the score is ΣU · Σ_k r_k): every score is
    NaN, and NaN ranks by column in both orders."""
    prob = grid_ref_problem(64, 10)
    assert prob.flags.ntn_mode == 'reference'
    off, size = _ntn_param(prob, 'weights_U')
    params = prob.params.copy()
    params[off + 3] = np.float32('nan')
    model = _edited_model(gpu, prob, params)
    eq, edb = _emb(gpu, 64, 3, 130)[:2]
    for final in (False, True):
        for k in (5, 64):
            v = _check_order(model, eq, edb, k, final)
            assert np.isnan(v).all()
        for largest in (True, False):
            idx, val = model.web_search(eq, edb, 64, largest=largest, final=final, seg_cols=64)
            assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(64), (3, 1)))
            assert np.isnan(val.cpu().numpy()).all()


# ---- 6. strides -------------------------------------------------------------------------------------
def test_web_search_strides(gpu):
    """Embeddings in the layout of the web_embed view (row stride 128 at D = 64, the columns
    past D never read: they hold NaN here) and as contiguous copies give the same bits; a
    query tensor of one row."""
    import torch
    model = _head(gpu, 64, 10)[0]
    eq, edb = _emb(gpu, 64, 5, 200)[:2]

    def strided(e):
        buf = torch.full((e.shape[0], 128), float('nan'), dtype=torch.float32, device=gpu)
        buf[:, :64] = e
        view = buf[:, :64]
        assert view.stride(0) == 128 and view.stride(1) == 1 and not view.is_contiguous()
        return view

    sq, sdb = strided(eq), strided(edb)
    for k, seg in ((5, 64), (64, 0)):
        want = _two_call(model, eq, edb, k, True, True)
        assert not torch.isnan(want[1]).any()
        for q, db in ((sq, sdb), (sq, edb), (eq, sdb)):
            assert _same(model.web_search(q, db, k, seg_cols=seg), want), (k, seg)
        assert _same(_two_call(model, sq, sdb, k, True, True), want)
        one = model.web_search(sq[2:3], sdb, k, seg_cols=seg)
        assert tuple(one[0].shape) == (1, k)
        assert _same(one, (want[0][2:3], want[1][2:3]))


# ---- 7. against the float64 head, independently of the grid kernel ---------------------------
@pytest.mark.parametrize('D,K', [(64, 10), (512, 16)])
def test_web_search_against_float64_head(gpu, D, K):
    head = _head(gpu, D, K)
    model = head[0]
    m, n, k = 5, 200, 5
    eq_t, edb_t, eq, edb = _emb(gpu, D, m, n)
    want = _ref(head, eq, edb)                            # pre-activation, float64
    bar = lambda x: TOL * (1.0 + np.abs(x))               # noqa: E731
    ranked = np.sort(want, axis=1)
    for largest in (True, False):
        for seg in (64, 0):
            idx, val = model.web_search(eq_t, edb_t, k, largest=largest, final=False,
                                        seg_cols=seg)
            idx = idx.cpu().numpy().astype(np.int64)
            val = val.cpu().numpy().astype(np.float64)
            at = np.take_along_axis(want, idx, axis=1)
            dev = np.abs(val - at)
            print('D', D, 'largest', largest, 'seg', seg, 'max |value - float64 head|',
                  float(dev.max()), 'max of it over the bar', float((dev / bar(at)).max()),
                  'max |score|', float(np.abs(want).max()))
            assert np.all(dev <= bar(at))
            assert all(len(set(r)) == k for r in idx)
            # the k-th returned column against the reference's (k + 1)-th best: twice the
            # bar, taken at the smaller of the two scores
            kth = at[:, k - 1]
            nxt = ranked[:, ::-1][:, k] if largest else ranked[:, k]
            slack = 2 * np.minimum(bar(kth), bar(nxt))
            assert np.all(kth >= nxt - slack) if largest else np.all(kth <= nxt + slack)


# ---- 8. end to end -----------------------------------------------------------------------------------
def test_web_embedding_index_nearest(gpu):
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.retrieval import EmbeddingIndex
    prob = _alive(sized_problem(_counts([1, 64], 64, 23, 5), ntn_stack(64, 10, dropout=0.0),
                                n_max=64, seed=21))
    model = gpu_model(prob, gpu)
    assert model.is_web
    db, queries = prob.mgs[:20], prob.mgs[20:]
    index = EmbeddingIndex(model, db)
    assert index.embeddings.stride(0) == 128             # the web_embed view is passed on
    for k in (1, 4, 20):
        for largest in (True, False):
            idx, sims = index.topk(queries, k, largest=largest)
            idx2, sims2 = index.nearest(queries, k, largest=largest)
            assert tuple(idx2.shape) == (5, k)
            assert torch.equal(idx, idx2) and torch.equal(sims.view(torch.int32),
                                                          sims2.view(torch.int32))
    with pytest.raises(_lib.SiameseHipError, match='nearest'):
        index.search(queries, 4)
    # a model off the graph-store path: nearest is search
    small = sized_problem([3, 5, 8, 2, 9, 4, 7], dict(dropout=0.0), n_max=10, seed=2)
    sm = gpu_model(small, gpu)
    assert not sm.is_web
    si = EmbeddingIndex(sm, small.mgs[:5])
    for k in (1, 5):
        a, b = si.nearest(small.mgs[4:], k), si.search(small.mgs[4:], k)
        assert _same(a, b) and _same(a, si.topk(small.mgs[4:], k))
    with pytest.raises(_lib.SiameseHipError):
        sm.web_search(np.zeros((1, 10), np.float32), np.zeros((1, 10), np.float32), 1)


# ---- 9. replay, streams, what is written ------------------------------------------------------------
def test_web_search_replay_stream_and_bounds(gpu):
    import torch
    from graphembedding_amd import _lib
    model = _head(gpu, 64, 10)[0]
    m, n, k, D = 6, 300, 7, 64
    eq, edb = _emb(gpu, D, m, n)[:2]
    want = _two_call(model, eq, edb, k, True, True)
    for seg in (0, 64):
        ws = torch.empty(_lib.web_search_workspace_bytes(model.sg, m, n, k, seg) // 4 + 1,
                         dtype=torch.float32, device=gpu)
        pad = 16
        ibuf = torch.full((m * k + 2 * pad,), -77, dtype=torch.int32, device=gpu)
        vbuf = torch.full((m * k + 2 * pad,), -7.25, dtype=torch.float32, device=gpu)
        idx, val = ibuf[pad:pad + m * k], vbuf[pad:pad + m * k]

        def call(i, v, stream=None):
            _lib.web_search_topk(model.sg, eq, D, edb, D, m, n, model.params, True, k, True, seg,
                                 i, v, ws, stream=stream)

        side = torch.cuda.Stream(device=gpu)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(idx, val, side.cuda_stream)
        side.synchronize()
        first = (idx.clone().view(m, k), val.clone().view(m, k))
        assert _same(first, want), seg
        for buf, fill in ((ibuf, -77), (vbuf, -7.25)):
            assert torch.all(buf[:pad] == fill) and torch.all(buf[pad + m * k:] == fill)
        # again into the same buffers, on the current stream
        call(idx, val)
        torch.cuda.synchronize()
        assert _same((idx.view(m, k), val.view(m, k)), first), seg
        # val_out = NULL
        idx2 = torch.full((m, k), -1, dtype=torch.int32, device=gpu)
        call(idx2, None)
        assert torch.equal(idx2, first[0])
        for buf, fill in ((ibuf, -77), (vbuf, -7.25)):
            assert torch.all(buf[:pad] == fill) and torch.all(buf[pad + m * k:] == fill)
