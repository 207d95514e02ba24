"""The k nearest graphs under exact GED on the GPU (include/siamese_ged_knn.h): all six outputs
of sg_ged_knn equal tests/_ged_knn_restatement.py bit for bit on all four sets, for every k and
budget of the lists below; certified rows equal brute force over the exact grid; the outputs do
not depend on where a query or a database graph stands in the call, on its neighbours or on the
run; entries the call cannot serve; the Python layer."""
import numpy as np
import pytest

import _ged_knn_cases as KC
import _ged_knn_restatement as K

pytestmark = pytest.mark.gpu

BUDGETS = KC.CUT_BUDGETS + (KC.PROVE_BUDGET,)
NAMES = ('cols', 'ub', 'lb', 'certified', 'candidates', 'expansions')
VERIFY_WAVES = 2048                 # the verify launch of siamese_ged_knn.h


def _run(gpu, store, k, budget, q=None, db=None, **kw):
    from graphembedding_amd.ged import ged_knn
    out = ged_knn(store, q, db, k=k, exact_budget=budget, device=gpu, stats=True, **kw)
    return [t.cpu().numpy() for t in out]


def _same(got, want, what=''):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])


@pytest.mark.parametrize('name', KC.SETS)
def test_all_outputs_equal_the_restatement(gpu, name):
    store, ref = KC.store(name)
    G = len(store)
    ids = list(range(G))
    for k in (1, 3, G, 64):
        for budget in BUDGETS:
            got = _run(gpu, store, k, budget)
            want = ref.knn(ids, ids, k, budget)
            _same(got, want, (name, k, budget))
            cols, ub, lb, cert, cand, ex = got
            assert (cand >= min(k, G)).all() and (cand <= G).all() and (ex >= 0).all()
            if budget == 0:
                assert not ex.any()
            if budget == KC.PROVE_BUDGET and name != 'cap32':
                assert cert.all() and np.array_equal(ub[:, :min(k, G)], lb[:, :min(k, G)])
            if k >= G:
                assert (cand == G).all() and (cols[:, G:] == -1).all()
    if name == 'knn24':                 # the branches test_ged_knn_host.py shows are reached
        cand, ex = _run(gpu, store, 3, KC.PROVE_BUDGET)[4:]
        assert (cand < G).any() and ex.sum() > 0
    if name == 'cap32':
        cert = _run(gpu, store, G, KC.PROVE_BUDGET)[3]
        assert not cert.all()


@pytest.mark.parametrize('name', KC.SETS)
def test_certified_rows_equal_brute_force_over_the_exact_grid(gpu, name):
    """cap32: the exact grid leaves pairs unproven (more than 16 nodes, or the budget), so only
    the certified rows whose whole exact row is proven can be sorted: the 1-node graph's row, at
    every k (the restatement shows both on the host)."""
    from graphembedding_amd.ged import ged_grid
    store, _ = KC.store(name)
    G = len(store)
    eub, elb = (t.cpu().numpy() for t in ged_grid(store, bounds=True, device=gpu,
                                                  exact_budget=KC.PROVE_BUDGET))
    whole = (eub == elb).all(axis=1)
    assert whole.all() or name == 'cap32'
    compared = 0
    for k in (1, 3, G, 64):
        cols, ub, lb, cert = _run(gpu, store, k, KC.PROVE_BUDGET)[:4]
        assert cert.all() or name == 'cap32'
        for i in range(G):
            if not (cert[i] and whole[i]):
                continue
            compared += 1
            want = K.brute_force_topk(list(eub[i]), k)
            assert list(cols[i]) == want, (k, i)
            assert list(ub[i, :min(k, G)]) == [eub[i, j] for j in want[:G]]
    assert compared >= (4 if name == 'cap32' else 4 * G)


def test_rows_do_not_depend_on_their_position(gpu):
    store, ref = KC.store('knn24')
    G = len(store)
    for k, budget in ((3, KC.PROVE_BUDGET), (5, 7)):
        full = _run(gpu, store, k, budget)
        rng = np.random.default_rng(k)
        q = np.concatenate([rng.permutation(G), rng.integers(0, G, size=13)])
        got = _run(gpu, store, k, budget, q)
        _same(got, [f[q] for f in full], 'permuted')
        again = _run(gpu, store, k, budget, q)            # two runs: bitwise equal
        _same(again, got, 'again')
        one = _run(gpu, store, k, budget, [7])            # m = 1
        _same(one, [f[[7]] for f in full], 'm=1')
        _same(_run(gpu, store, k, budget, [7], [4]),      # m = 1 and n = 1
              ref.knn([7], [4], k, budget), 'n=1')


def test_unservable_columns_between_the_others_take_no_part(gpu):
    import copy

    from graphembedding_amd import _lib
    store, ref = KC.store('knn24')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    k, budget = 3, 1000
    db = np.arange(2 * G)
    db[1::2] = np.array([-1, 4, G, 2 ** 31 - 1] * (G // 4))   # every second column unservable
    db[0::2] = np.arange(G)
    db[8] = 5                                                 # graph 4 itself is holed: any other
    good = np.flatnonzero((db >= 0) & (db < G) & (db != 4))
    q = np.array([3, 9, 20])
    got = _run(gpu, holed, k, budget, q, db, return_status=True)
    assert int(got[6][0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    want = K.KnnReference(holed).knn(q, db, k, budget)
    _same(got[:6], want, 'holed')
    dense = _run(gpu, store, k, budget, q, db[good])          # the same columns, packed
    assert np.array_equal(good[dense[0]], got[0])
    for a, b in zip(dense[1:], got[1:6]):
        assert np.array_equal(a, b)
    assert np.isin(got[0], good).all()


def test_unservable_queries_read_minus_one_and_set_the_status(gpu):
    import copy

    from graphembedding_amd import _lib
    from graphembedding_amd.ged import ged_knn
    store, _ = KC.store('cap10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    q = np.array([3, -1, 7, 4, G, 6])
    db = np.array([9, 4, 3, 2 ** 31 - 1, 7, 5])
    got = _run(gpu, holed, 4, 1000, q, db, return_status=True)
    assert int(got[6][0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    _same(got[:6], K.KnnReference(holed).knn(q, db, 4, 1000), 'holed')
    cols, ub, lb, cert, cand, ex = got[:6]
    bad = [1, 3, 4]
    assert (cols[bad] == -1).all() and (ub[bad] == -1).all() and (lb[bad] == -1).all()
    assert not cert[bad].any() and (cand[bad] == -1).all() and (ex[bad] == -1).all()
    assert (cols[[0, 2, 5]] >= 0).all() and (cand[[0, 2, 5]] >= 4).all()
    none = _run(gpu, holed, 2, 7, [3], [4, -1], return_status=True)   # no servable column
    assert (none[0] == -1).all() and none[3][0] == 1 and none[4][0] == 0 and none[5][0] == 0
    assert int(_run(gpu, holed, 2, 7, [0, G], [1], return_status=True)[6][0]) == _lib.SG_ERR_ARG
    assert int(_run(gpu, holed, 2, 7, [0, 4], [1], return_status=True)[6][0]) == _lib.SG_ERR_SHAPE
    assert int(_run(gpu, holed, 2, 7, [0, 3], [1], return_status=True)[6][0]) == 0
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_knn: SG_ERR_SHAPE'):
        ged_knn(holed, [4], [1], k=1, exact_budget=7, device=gpu)
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_knn: SG_ERR_ARG'):
        ged_knn(holed, [0], [G], k=1, exact_budget=7, device=gpu)


def test_a_long_row_and_a_grid_the_verify_launch_strides_over(gpu):
    """1 x 4096 by repeating knn24: a graph's 170 copies tie in every bound, so the column order
    decides and the row spans 16 passes of its workgroup.  Then 192 x 48 (every query 8 times,
    every database graph twice, k = 6: the thresholds of the all-pairs k = 3), which lists more
    candidates than the verify launch has wavefronts, most of them searched."""
    store, ref = KC.store('knn24')
    G = len(store)
    db = np.arange(4096) % G
    for k, budget in ((3, 1000), (64, 7)):
        got = _run(gpu, store, k, budget, [11], db)
        _same(got, ref.knn([11], db, k, budget), ('1x4096', k))
        assert got[4][0] >= 4096 // G
    q, db = np.arange(8 * G) % G, np.arange(2 * G) % G
    k, budget = 6, 1000
    got = _run(gpu, store, k, budget, q, db)
    _same(got, ref.knn(q, db, k, budget), '192x48')
    assert got[4].sum() > VERIFY_WAVES and got[5].sum() > VERIFY_WAVES
    again = _run(gpu, store, k, budget, q, db)
    _same(again, got, 'again')


def test_the_python_layer(gpu):
    from graphembedding_amd import ged
    from graphembedding_amd.ged import csr_store_of_graphs
    store, ref = KC.store('knn24')
    graphs = KC.graphs('knn24')
    G = len(store)
    out = ged.ged_knn(store, k=3, exact_budget=KC.PROVE_BUDGET, device=gpu)
    assert len(out) == 4 and all(t.is_cuda for t in out)
    assert [t.dtype for t in out] == [__import__('torch').int32] * 4
    assert out[0].shape == (G, 3) and out[3].shape == (G,)
    assert len(ged.ged_knn(store, k=3, exact_budget=7, device=gpu, return_status=True)) == 5
    assert len(ged.ged_knn(store, k=3, exact_budget=7, device=gpu, stats=True)) == 6
    with pytest.raises(ValueError, match='CSR'):
        ged.ged_knn(csr_store_of_graphs(graphs), k=3, device=gpu)
    with pytest.raises(ValueError, match='k 65'):
        ged.ged_knn(store, k=65, device=gpu)
    # networkx in, numpy out: the last five graphs as queries against the first nineteen
    cols, dist, proven, cert = ged.ged_knn_graphs(graphs[:19], graphs[19:], k=4,
                                                  exact_budget=KC.PROVE_BUDGET, device=gpu)
    want = ref.knn(range(19, G), range(19), 4, KC.PROVE_BUDGET)
    assert cols.dtype == np.int64 and dist.dtype == np.int64 and proven.dtype == bool
    assert np.array_equal(cols, want[0]) and np.array_equal(dist, want[1])
    assert np.array_equal(proven, want[1] == want[2]) and np.array_equal(cert, want[3] == 1)
    # a perfect index has recall 1, one that returns the farthest graphs has less
    true = out[0]
    assert ged.knn_recall(true, true, out[3]) == (1.0, G)
    far = np.argsort(-ref.exact.grid(range(G), range(G), KC.PROVE_BUDGET)[0], axis=1)[:, :3]
    r, rows = ged.knn_recall(far, true, out[3])
    assert rows == G and r < 0.5
