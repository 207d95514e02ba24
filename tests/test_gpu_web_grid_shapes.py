"""The launch shapes of embed-once retrieval for graph-store (Web) models that
test_gpu_web_embed.py never reaches (include/siamese_web_embed.h).

sg_web_score_grid: more than one query tile pair and the absent second tile, table row chunks
of more than 16 rows (ragged, and at the clamp of 8), workgroups that walk more than four
queries through the double-buffered LDS pipeline, every A-operand instantiation and both sides
of each of their boundaries, D % 4 in {1, 3}, D = 32.  The embeddings are synthetic (dense,
signed: _embed_fixtures.signed_embeddings), so every W[a][b][k] counts, and the scores are
measured against the float64 head of _embed_fixtures.ntn_head_ref, which test_web_grid_ref.py
checks on the CPU.  Tolerance: the project's per-pair 1e-4, rtol = atol.

sg_web_embed: the size-class sort over two blocks, the 128 / 129 and 256 / 257 class
boundaries at D = 512, and the device status SG_ERR_SHAPE."""
import numpy as np
import pytest

from _embed_fixtures import (GRID_REF_MODELS, gpu_model, grid_ref_embeddings, grid_ref_problem,
                             ntn_head_params, ntn_head_ref, ntn_stack, sized_problem)
from test_gpu_web_embed import _alive, _counts, _csr, _grid, _oracle_embeddings, _raw

pytestmark = pytest.mark.gpu

TOL = 1e-4


# ---- what the host code of sg_web_score_grid decides from (m, n, D, CUs) -------------------
# A transcription of grid_split (sg_embed_plan.h) and of the table chunk formula
# (sg_web_grid.hip).  It only guards coverage: each case asserts that it reaches the
# configuration it is meant to before it calls the kernel.  It is never a reference for a
# result: those come from ntn_head_ref and from calls at other launch shapes.
def _cus(gpu):
    import torch
    return int(torch.cuda.get_device_properties(gpu).multi_processor_count)


def _grid_split(m, n, target):
    ncb = (n + 63) // 64
    nqc = max(1, min((target + ncb - 1) // max(ncb, 1), (m + 3) // 4))
    qb = max(4, (((m + nqc - 1) // nqc) + 3) & ~3)
    nqc = (m + qb - 1) // qb
    return dict(ncb=ncb, nqc=nqc, qb=qb, last=m - (nqc - 1) * qb)


def _table_chunks(m, D, cus):
    Dq = (D + 1 + 3) & ~3
    mt, nb16 = (m + 31) // 32, (Dq + 15) // 16
    raw = mt * nb16 // (2 * cus)
    R = min(8, max(1, raw))
    bch = 16 * R
    return dict(Dq=Dq, mt=mt, raw=raw, R=R, bch=bch, nbc=(Dq + bch - 1) // bch,
                ragged=Dq % bch != 0)


def _nsmax(D):
    """(ns, the instantiation web_grid_kernel<NSMAX> that serves it)"""
    ns = ((D + 1 + 3) & ~3) // 4
    return ns, next(x for x in (17, 33, 65, 97, 129) if ns <= x)


# ---- models, embeddings, calls ------------------------------------------------------------
_HEADS = {}


def _head(gpu, D, K, bias=True, ntn_mode='reference'):
    """(model, (W, V, bias, U) in float64) of a model of GRID_REF_MODELS: built once."""
    key = (D, K, bias, ntn_mode)
    assert key in GRID_REF_MODELS      # the sensitivity condition of test_web_grid_ref.py holds
    if key not in _HEADS:
        prob = grid_ref_problem(D, K, bias, ntn_mode)
        model = gpu_model(prob, gpu)
        assert model.is_web and model.web_embed_dim == D and model.sg.keep_prob == 1.0
        _HEADS[key] = (model, ntn_head_params(prob), ntn_mode, K)
    return _HEADS[key]


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _ref(head, eq, edb, final_act=None):
    _, (W, V, b, U), mode, K = head
    return ntn_head_ref(eq, edb, W, V, b, U, mode, K, final_act)


def _close(tag, got, ref):
    print(tag, 'max |grid - float64 head|', float(np.abs(got - ref).max()),
          'max |score|', float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=TOL, atol=TOL)


def _one_by_one(model, eq_t, edb_t, rows):
    """The rows `rows` of the grid from calls of m = 1 each."""
    return np.concatenate([_grid(model, eq_t[i:i + 1], edb_t, False, 3) for i in rows])


def _by_cuts(model, eq_t, edb_t, cut=64):
    """The grid from calls over at most `cut` database rows each."""
    n = int(edb_t.shape[0])
    return np.concatenate([_grid(model, eq_t, edb_t[j:j + cut], False, 3)
                           for j in range(0, n, cut)], axis=1)


# ---- query-tile edges of the table kernel ---------------------------------------------------
_SINGLE = {}


@pytest.mark.parametrize('m', [16, 32, 33, 48, 49, 65])
def test_query_tile_edges(gpu, m):
    """m = 16 and 32 fill the tiles of one pair exactly; 33 and 48 leave the second tile of the
    second pair absent (i0 = 32, i0 + 16 >= m); 49 has it with one query; 65 has three pairs,
    the last with one query.  Every row is the row of an m = 1 call, bit for bit."""
    D, K, n = 64, 10, 3
    head = _head(gpu, D, K)
    model = head[0]
    cfg = _table_chunks(m, D, _cus(gpu))
    i0_last = 32 * (cfg['mt'] - 1)
    two_last = i0_last + 16 < m
    want = {16: (1, False), 32: (1, True), 33: (2, False), 48: (2, False), 49: (2, True),
            65: (3, False)}[m]
    assert (cfg['mt'], two_last) == want and cfg['R'] == 1
    eq, edb = grid_ref_embeddings(D, 65, n)              # rows [:m] are the case's queries
    eq_t, edb_t = _dev(eq, gpu), _dev(edb, gpu)
    if 'rows' not in _SINGLE:
        _SINGLE['rows'] = _one_by_one(model, eq_t, edb_t, range(65))
    got = _grid(model, eq_t[:m], edb_t, False, 3)
    _close('tile edges D 64 m {}'.format(m), got, _ref(head, eq[:m], edb))
    assert np.array_equal(got, _SINGLE['rows'][:m])


# ---- workgroups that walk more than four queries --------------------------------------------
def _odd_chunk_m(n, cus):
    """The first odd m >= 41 whose split has qb > 4 and an odd last chunk of more than 4."""
    for m in range(41, 41 + 64, 2):
        s = _grid_split(m, n, 2 * cus)
        if s['qb'] > 4 and s['last'] > 4 and s['last'] % 2 == 1:
            return m, s
    pytest.fail('no m in [41, 105) walks an odd chunk of more than 4 queries at n = {}'.format(n))


@pytest.mark.parametrize('D,K', [(64, 10), (512, 16)])
@pytest.mark.parametrize('n_per_cu', [32, 128])
def test_multi_query_chunks(gpu, D, K, n_per_cu):
    """n = 32 CUs + 1: fewer column blocks than the 2 CUs target, so the queries are cut into
    chunks of qb = 12 with a last chunk of 5 (at 256 CUs).  n = 128 CUs + 1: more column blocks
    than the target, one chunk walks all 41 queries (qb = 44): the last query of an odd count
    sits in buffer 0 after a full pipeline.  The last column block has one valid row.
    Against the float64 head, and bit for bit against calls of n <= 64, which run at qb = 4."""
    cus = _cus(gpu)
    n = n_per_cu * cus + 1
    m, s = _odd_chunk_m(n, cus)
    print('D', D, 'm', m, 'n', n, 'CUs', cus, s)
    assert s['qb'] > 4 and s['last'] > 4 and s['last'] % 2 == 1 and n % 64 == 1
    if n_per_cu == 128:
        assert s['nqc'] == 1 and s['last'] == m          # a single chunk walks every query
    else:
        assert s['nqc'] > 1                              # full chunks, then the odd one
    assert _grid_split(m, 64, 2 * cus)['qb'] == 4 and _grid_split(m, 1, 2 * cus)['qb'] == 4
    head = _head(gpu, D, K)
    model = head[0]
    eq, edb = grid_ref_embeddings(D, m, n)
    eq_t, edb_t = _dev(eq, gpu), _dev(edb, gpu)
    got = _grid(model, eq_t, edb_t, False, 3)
    _close('chunks D {} m {} n {} qb {}'.format(D, m, n, s['qb']), got, _ref(head, eq, edb))
    assert np.array_equal(got, _by_cuts(model, eq_t, edb_t))


# ---- table row chunks -------------------------------------------------------------------------
def _row_chunk_case(gpu, D, K, m, n, check):
    head = _head(gpu, D, K)
    model = head[0]
    cfg = _table_chunks(m, D, _cus(gpu))
    print('D', D, 'm', m, cfg, 'NSMAX', _nsmax(D))
    check(cfg)
    eq, edb = grid_ref_embeddings(D, m, n)
    eq_t, edb_t = _dev(eq, gpu), _dev(edb, gpu)
    got = _grid(model, eq_t, edb_t, False, 3)
    _close('row chunks D {} m {} R {}'.format(D, m, cfg['R']), got, _ref(head, eq, edb))
    # 64 rows: the first tile pair (both tiles), the middle, the last tile pair and its
    # neighbour (m = 32 mt - 15: the last pair holds 17 queries)
    mid = (m // 2) & ~31
    rows = list(range(22)) + list(range(mid + 6, mid + 27)) + list(range(m - 21, m))
    assert len(set(rows)) == 64 and m - 21 < 32 * (cfg['mt'] - 1) < m - 1
    assert np.array_equal(got[rows], _one_by_one(model, eq_t, edb_t, rows))


def test_table_row_chunks_r3(gpu):
    """R = 3: chunks of 48 table rows, the last one ragged (Dq = 260 = 5 x 48 + 20); ns = 65 is
    also the last width web_grid_kernel<65> serves."""
    cus = _cus(gpu)
    mt = -(-6 * cus // 17)

    def check(cfg):
        assert cfg['mt'] == mt and cfg['R'] == 3 and cfg['bch'] == 48 and cfg['Dq'] == 260
        assert cfg['nbc'] == 6 and cfg['ragged']
        assert _nsmax(256) == (65, 65)
    _row_chunk_case(gpu, 256, 10, 32 * mt - 15, 3, check)


def test_table_row_chunks_clamped(gpu):
    """mt nb16 / (2 CUs) >= 9: the clamp acts, R = 8, chunks of 128 rows, the last ragged
    (Dq = 516 = 4 x 128 + 4).  D = 512, K = 16: a table workspace of about 150 MB."""
    cus = _cus(gpu)
    mt = -(-18 * cus // 33)

    def check(cfg):
        assert cfg['mt'] == mt and cfg['raw'] >= 9 and cfg['R'] == 8 and cfg['bch'] == 128
        assert cfg['Dq'] == 516 and cfg['nbc'] == 5 and cfg['ragged']
    _row_chunk_case(gpu, 512, 16, 32 * mt - 15, 2, check)


# ---- widths and instantiations ----------------------------------------------------------------
# D: (ns, NSMAX).  32 is the smallest width; 33 has D % 4 = 1 (two zero rows), 63, 67 and
# 127 D % 4 = 3 (Dq = D + 1: the bias row is the last table row, no zero rows); 67 | 68,
# 127 | 132, 256 | 260 and 384 | 388 are the two sides of the four instantiation boundaries.
WIDTHS = {32: (9, 17), 33: (9, 17), 63: (16, 17), 67: (17, 17), 68: (18, 33), 127: (32, 33),
          132: (34, 65), 256: (65, 65), 260: (66, 97), 384: (97, 97), 388: (98, 129)}
WIDTH_CASES = ([(D, 10, True, 'reference') for D in WIDTHS] +
               [(63, 16, False, 'reference'), (127, 16, False, 'reference'),
                (260, 10, True, 'intended')])


@pytest.mark.parametrize('D,K,bias,ntn_mode', WIDTH_CASES)
def test_widths_and_instantiations(gpu, D, K, bias, ntn_mode):
    assert _nsmax(D) == WIDTHS[D]
    if D in (63, 127):
        assert (D + 1 + 3) & ~3 == D + 1
    head = _head(gpu, D, K, bias, ntn_mode)
    model = head[0]
    eq, edb = grid_ref_embeddings(D, 5, 37)
    eq_t, edb_t = _dev(eq, gpu), _dev(edb, gpu)
    got = _grid(model, eq_t, edb_t, False, 3)
    tag = 'widths D {} K {} bias {} {}'.format(D, K, bias, ntn_mode)
    _close(tag, got, _ref(head, eq, edb))
    act = _grid(model, eq_t, edb_t, True, 3)
    np.testing.assert_allclose(act, _ref(head, eq, edb, model.apply_final_act_np),
                               rtol=TOL, atol=TOL)


# ---- the dense embeddings reach W at high indices -----------------------------------------------
@pytest.mark.parametrize('D,K', [(64, 10), (512, 16)])
def test_last_component_is_live(gpu, D, K):
    """Flipping the sign of component a = D - 1 of one query moves every score of its row of
    the float64 head by more than 10 TOL (with the real, non-negative embeddings that are zero
    past a graph's node count it would move none), and the kernel follows."""
    head = _head(gpu, D, K)
    eq, edb = grid_ref_embeddings(D, 5, 37)
    flipped = eq.copy()
    flipped[2, D - 1] = -flipped[2, D - 1]
    ref, ref_f = _ref(head, eq, edb), _ref(head, flipped, edb)
    moved = np.abs(ref_f - ref)
    print('D', D, 'row 2 moves by', float(moved[2].min()), '..', float(moved[2].max()))
    assert np.all(moved[2] > 10 * TOL) and not moved[[0, 1, 3, 4]].any()
    got = _grid(head[0], _dev(flipped, gpu), _dev(edb, gpu), False, 3)
    _close('flipped D {}'.format(D), got, ref_f)


# ---- sg_web_embed ---------------------------------------------------------------------------------
_EMBED = {}


def _embed_case(name, gpu):
    """(problem, model, CSR store, oracle embeddings): built once, read only."""
    if name not in _EMBED:
        if name == 'd64':
            counts, D, K, n_types = _counts([1, 16, 17, 32, 33, 64], 64, 34, 8), 64, 10, 29
        else:
            counts, D, K, n_types = [1, 128, 129, 256, 257, 512], 512, 16, 60
        prob = _alive(sized_problem(counts, ntn_stack(D, K, dropout=0.0), n_max=D, seed=11,
                                    n_types=n_types))
        model = gpu_model(prob, gpu)
        assert model.is_web and model.web_embed_dim == D
        _EMBED[name] = (prob, model, _csr(prob, model), _oracle_embeddings(prob))
    return _EMBED[name]


def _size_class(n, n_max):
    """Transcribed from sg_web_embed (coverage guard only): 0, 1 or 2."""
    n16 = (n_max + 15) & ~15
    cap4, cap2 = (n16 // 4) & ~15, (n16 // 2) & ~15
    return 0 if n <= cap4 else (1 if n <= cap2 else 2)


def test_web_embed_two_sort_blocks(gpu):
    """4096 + 37 entries: the size-class sort runs over two blocks (kUnitChunk = 4096), each
    with all three classes.  A graph's row is that of a one-graph call, bit for bit."""
    from graphembedding_amd import _lib
    prob, model, store, ref = _embed_case('d64', gpu)
    G, D = len(store), 64
    assert G == 40 and {1, 16, 17, 32, 33, 64} <= set(int(x) for x in store.n)
    idx = np.random.default_rng(5).integers(0, G, size=4096 + 37)
    assert (len(idx) + 4095) // 4096 == 2                # nbu
    cls = np.array([_size_class(int(store.n[g]), store.n_max) for g in idx])
    for blk in (cls[:4096], cls[4096:]):
        assert set(blk) == {0, 1, 2}
    ld = _lib.web_embed_ld(model.sg)
    e_t = model.web_embed(store, idx)
    e = e_t.cpu().numpy()
    assert e.shape == (len(idx), D)
    print('two sort blocks max |emb - oracle|', float(np.abs(e - ref[idx]).max()))
    np.testing.assert_allclose(e, ref[idx], rtol=TOL, atol=TOL)
    single = np.concatenate([model.web_embed(store, [g]).cpu().numpy() for g in range(G)])
    assert np.array_equal(e, single[idx])
    assert not _raw(e_t, ld).cpu().numpy()[:, D:].any()  # columns [D, ld) zero


def test_web_embed_size_classes_d512(gpu):
    """Node counts on both sides of cap4 = 128 and cap2 = 256 at the widest width, in this
    order, reversed, and one graph per call: the same bits."""
    prob, model, store, ref = _embed_case('d512', gpu)
    assert [int(x) for x in store.n] == [1, 128, 129, 256, 257, 512] and store.n_max == 512
    assert [_size_class(int(x), 512) for x in store.n] == [0, 0, 1, 1, 2, 2]
    e = model.web_embed(store).cpu().numpy()
    print('d512 size classes max |emb - oracle|', float(np.abs(e - ref).max()))
    assert all((ref[i, :int(n)] != 0).mean() > 0.5 for i, n in enumerate(store.n))
    np.testing.assert_allclose(e, ref, rtol=TOL, atol=TOL)
    rev = model.web_embed(store, np.arange(6)[::-1].copy()).cpu().numpy()
    assert np.array_equal(rev[::-1], e)
    for g in range(6):
        assert np.array_equal(model.web_embed(store, [g]).cpu().numpy()[0], e[g])


def _embed_raw(model, store, idx, gpu):
    """sg_web_embed with a status word into a buffer filled with 7: (rows [len(idx)][ld],
    device status)."""
    import torch
    from graphembedding_amd import _lib
    ld = _lib.web_embed_ld(model.sg)
    idx_t = torch.as_tensor(np.asarray(idx, np.int64), dtype=torch.int32, device=gpu)
    out = torch.full((len(idx), ld), 7.0, dtype=torch.float32, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(_lib.web_embed_workspace_bytes(model.sg, len(idx)) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    _lib.web_embed(model.sg, store.to_device(gpu), idx_t, len(idx), model.params, out, ws, status)
    return out.cpu().numpy(), int(status.item())


def test_web_embed_shape_status(gpu):
    """A graph of the store with more than store->n_max nodes, and one with none, raise
    SG_ERR_SHAPE in the device status and give a zero row; the other rows keep their bits.
    Both get the empty record in web_embed_inst_kernel before anything is read at their
    offsets, and every offset stays inside the store's arrays."""
    from graphembedding_amd import _lib
    prob, model, store, _ = _embed_case('d64', gpu)
    G = len(store)
    ns = [int(x) for x in store.n]
    big = [g for g in range(G) if ns[g] == 64]
    fit = [g for g in range(G) if ns[g] < 64]
    assert big and len(fit) > 30 and 33 in [ns[g] for g in fit]
    good, st = _embed_raw(model, store, list(range(G)), gpu)
    assert st == 0 and good.any(axis=1).all()

    # (a) n_max lowered below the largest graph (63: the size classes keep their bounds)
    low = _csr(prob, model)
    low.n_max = 63
    assert _size_class(16, 63) == 0 and _size_class(17, 63) == 1 and _size_class(33, 63) == 2
    ids = [fit[0], big[0], fit[1], fit[2], big[-1], fit[3], fit[4]]
    out, st = _embed_raw(model, low, ids, gpu)
    assert st == _lib.SG_ERR_SHAPE
    assert not out[1].any() and not out[4].any()
    assert np.array_equal(out[[0, 2, 3, 5, 6]], good[[ids[i] for i in (0, 2, 3, 5, 6)]])
    out, st = _embed_raw(model, low, fit, gpu)               # nothing too large: no status
    assert st == 0 and np.array_equal(out, good[fit])
    out, st = _embed_raw(model, low, [big[0]], gpu)          # nothing else in the call
    assert st == _lib.SG_ERR_SHAPE and not out.any()
    # an id outside the store and a graph too large: either code, both rows zero
    out, st = _embed_raw(model, low, [fit[0], G + 5, big[0], fit[1]], gpu)
    assert st in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    assert not out[1].any() and not out[2].any()
    assert np.array_equal(out[[0, 3]], good[[fit[0], fit[1]]])

    # (b) node_off repeats an offset: a graph with no nodes, in the middle and at the end
    hole = _csr(prob, model)
    k = 7
    total = int(hole.node_off[-1])
    hole.node_off = np.concatenate([hole.node_off[:k + 1], hole.node_off[k:],
                                    [total]]).astype(np.int32)
    hole.n = np.diff(hole.node_off).astype(np.int32)
    assert len(hole) == G + 2 and hole.n[k] == 0 and hole.n[-1] == 0
    assert [int(x) for x in np.delete(hole.n, [k, G + 1])] == ns
    assert hole.node_off.max() == total and hole.row_ptr.shape[0] == total + 1
    old = [g for g in range(G + 2) if g not in (k, G + 1)]  # new id -> the untouched store's
    out, st = _embed_raw(model, hole, list(range(G + 2)), gpu)
    assert st == _lib.SG_ERR_SHAPE
    assert not out[k].any() and not out[G + 1].any()
    assert np.array_equal(out[old], good)
    out, st = _embed_raw(model, hole, old, gpu)
    assert st == 0 and np.array_equal(out, good)
