"""sg_mcs_grid where tests/test_gpu_mcs.py does not reach (the sets of tests/_mcs_classes.py;
test_mcs_classes_host.py proves on the host what is relied on here): states of up to 32
classes, edgeless, disconnected and dense graphs, store capacities 1, 2, 3, 17 and 31, budgets
within one expansion of a pair's need and the largest legal one, grids of many workgroups per
compute unit, and adjacency weights and type ids that are not 0/1 and small.  All five outputs
equal tests/_mcs_restatement.py bit for bit; the closed forms and planted bounds of
_mcs_classes.known and the maps recomputed from the store arrays need no restatement."""
import copy

import numpy as np
import pytest

import _ged_classes as K
import _mcs_cases as C
import _mcs_classes as M
import _mcs_restatement as X
from test_gpu_mcs import _all_pairs, _check_map, _plain, _run, _want

pytestmark = pytest.mark.gpu

CASES = [(name, b, c) for name in M.SETS for b in M.budgets(name) for c in (False, True)]
_OUT = {}


def _set(gpu, name, budget, connected):
    """All pairs of a set of _mcs_classes.py, one call per (set, budget, connected)."""
    key = (name, budget, connected)
    if key not in _OUT:
        _OUT[key] = _run(gpu, M.store(name)[0], budget, connected)
    return _OUT[key]


def _equal(got, want):
    for g, w, what in zip(got, want, ('size', 'bound', 'edges', 'map', 'expansions')):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert np.array_equal(g, w), (what, np.argwhere(g != w)[:5])


# ---- 1. classes and capacities ------------------------------------------------------------
@pytest.mark.parametrize('name,budget,connected', CASES,
                         ids=['{}-{}-{}'.format(n, b, 'conn' if c else 'any') for n, b, c in CASES])
def test_classes_and_capacities_equal_the_restatement(gpu, name, budget, connected):
    store, ref = M.store(name)
    G = len(store)
    prove = M.PROVE_BUDGET[name]
    ref.grid(range(G), range(G), connected, prove)      # one search a pair serves every budget
    got = _set(gpu, name, budget, connected)
    size, bound, ed, mp, ex = got
    assert size.dtype == np.int32 and bound.dtype == np.int32 and ed.dtype == np.int32
    assert mp.dtype == np.int8 and ex.dtype == np.int64
    assert size.shape == bound.shape == ed.shape == ex.shape == (G, G)
    assert mp.shape == (G, G, store.n_max) and store.n_max == M.capacity(name)
    _equal(got, _want(ref, range(G), range(G), connected, budget))
    assert (ex <= budget).all() and (ex >= 0).all() and (size <= bound).all()
    if budget == 0:
        assert not ex.any() and not size.any()
    # every map, from the store's own arrays
    gs = [_plain(store, g) for g in range(G)]
    for a in range(G):
        for b in range(G):
            n1 = len(gs[a][0])
            assert (mp[a, b, n1:] == -1).all()
            phi = [int(x) for x in mp[a, b, :n1]]
            assert _check_map(gs[a], gs[b], phi, connected) == (size[a, b], ed[a, b]), (a, b)
    if budget != prove:
        return
    allowed = set(M.ALLOWED_UNPROVEN.get(name, ()))
    proven = size == bound
    assert {(int(a), int(b)) for a, b in np.argwhere(~proven)} == allowed
    assert ex[proven].max() <= budget // 2 and (ex[~proven] == budget).all()
    known = M.known(name)
    graphs = M.graphs(name)
    n_known = 0
    for (a, b, c), rule in known.items():
        if c == int(connected):
            assert M.holds(rule, size[a, b], proven[a, b]), (a, b, rule, size[a, b])
            n_known += 1
    assert connected or n_known >= G
    if name == 'edge0' and not connected:                # size = bound = ub0
        ub0 = np.array([[M.common_types(x, y) for y in graphs] for x in graphs])
        assert np.array_equal(size, ub0) and np.array_equal(bound, ub0)
    if name in K.PLANTED or name in M.WIDE:              # g against pi(g): an isomorphism
        for a, b in ((0, 1), (1, 0)):
            assert size[a, b] == bound[a, b] == store.n[a]
            assert K.is_isomorphism(graphs[a], graphs[b], [int(x) for x in mp[a, b]])
    both = proven & proven.T
    assert np.array_equal(size[both], size.T[both])      # symmetric where both are proven
    if connected:                                        # no larger than the unconnected one
        usize, ubound = _set(gpu, name, budget, False)[:2]
        both = proven & (usize == ubound)
        assert (size[both] <= usize[both]).all()


# ---- 2. budget edges ----------------------------------------------------------------------
_NEEDS = {}


def _one10_needs():
    """The proving needs of one10 and eight of the distinct ones: the smallest, the largest and
    six spread between them."""
    if not _NEEDS:
        needs = C.proving_expansions('one10')
        distinct = sorted(set(needs.values()))
        assert distinct[0] >= 1 and distinct[-1] == 318 and len(distinct) >= 8
        pick = sorted({int(round(x)) for x in np.linspace(0, len(distinct) - 1, 8)})
        assert len(pick) == 8
        _NEEDS['needs'], _NEEDS['chosen'] = needs, [distinct[i] for i in pick]
    return _NEEDS['needs'], _NEEDS['chosen']


@pytest.mark.parametrize('rank', range(8))
def test_budgets_one_below_and_at_a_pairs_need(gpu, rank):
    store, ref = C.store('one10')
    G = len(store)
    needs, chosen = _one10_needs()
    e = chosen[rank]
    n_hit = 0
    for connected in (False, True):
        below = _run(gpu, store, e - 1, connected)
        at = _run(gpu, store, e, connected)
        _equal(below, _want(ref, range(G), range(G), connected, e - 1))
        _equal(at, _want(ref, range(G), range(G), connected, e))
        for a in range(G):
            for b in range(G):
                if needs[(a, b, int(connected))] != e:
                    continue
                ub0 = X._rest(X.root_classes(ref.graph(a), ref.graph(b)))
                size, bound, _, _, ex = (x[a, b] for x in below)
                assert ex == e - 1 and size != bound and bound == ub0, (a, b, connected)
                size, bound, _, _, ex = (x[a, b] for x in at)
                assert ex == e and size == bound, (a, b, connected)
                n_hit += 1
    assert n_hit >= 1


@pytest.mark.parametrize('name', C.PROVEN_SETS)
def test_the_largest_legal_budget(gpu, name):
    """2^24: every pair of these sets proves within 318 expansions, so the call ends at once."""
    store, _ = C.store(name)
    assert X.MAX_BUDGET == 1 << 24
    for connected in (False, True):
        want = _all_pairs(gpu, name, C.PROVE_BUDGET, connected)
        assert np.array_equal(want[0], want[1]) and want[4].max() <= 318
        _equal(_run(gpu, store, X.MAX_BUDGET, connected), want)


# ---- 3. many workgroups per compute unit --------------------------------------------------
# 97 x 127 = 12,319 pairs, no multiple of the 4 pairs of a workgroup.  A workgroup holds
# 37,888 B of LDS; by an estimate nobody has measured, 160 KiB per compute unit hold 4 of them,
# so 256 compute units hold 4,096 pairs at once.  The grid is three times that and the test
# does not hinge on the exact figure: later workgroups start on LDS that earlier ones of this
# kernel left behind.
BIG = (97, 127)
BIG_LD = 131


def _big_ids(G):
    rng = np.random.default_rng(9712)
    return rng.integers(0, G, size=BIG[0]), rng.integers(0, G, size=BIG[1])


@pytest.mark.parametrize('connected', [False, True], ids=['any', 'conn'])
@pytest.mark.parametrize('budget', [100, C.PROVE_BUDGET])
def test_a_grid_of_many_workgroups_per_compute_unit(gpu, budget, connected):
    store, ref = C.store('one10')
    G = len(store)
    q, db = _big_ids(G)
    assert (BIG[0] * BIG[1]) % 4 and set(q) == set(db) == set(range(G))
    full = _all_pairs(gpu, 'one10', budget, connected)
    _equal(full, _want(ref, range(G), range(G), connected, budget))
    got = _run(gpu, store, budget, connected, q, db, ld=BIG_LD)
    _equal(got, [f[np.ix_(q, db)] for f in full])
    again = _run(gpu, store, budget, connected, q, db, ld=BIG_LD)
    _equal(again, got)
    if budget == 100:
        assert (got[4] == budget).any() and (got[4] < budget).any()


@pytest.mark.parametrize('budget,connected', [(100, False), (C.PROVE_BUDGET, True)])
def test_the_large_grid_with_unservable_entries(gpu, budget, connected):
    from graphembedding_amd import _lib
    store, _ = C.store('one10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    q, db = _big_ids(G)
    q, db = q.copy(), db.copy()
    q[[0, 55]] = (-1, G)
    db[[3, 64, 126]] = (4, -1, G)
    bad_q = (q < 0) | (q >= G) | (q == 4)
    bad_db = (db < 0) | (db >= G) | (db == 4)
    assert bad_q.sum() >= 3 and bad_db.sum() >= 4 and (~bad_q).sum() > 64
    full = _all_pairs(gpu, 'one10', budget, connected)
    size, bound, ed, mp, ex, status = _run(gpu, holed, budget, connected, q, db, ld=BIG_LD,
                                           return_status=True)
    assert int(status[0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    for out in (size, bound, ed, mp, ex):
        assert (out[bad_q] == -1).all() and (out[:, bad_db] == -1).all()
    gq, gdb = np.flatnonzero(~bad_q), np.flatnonzero(~bad_db)
    for out, f in zip((size, bound, ed, mp, ex), full):
        assert np.array_equal(out[np.ix_(gq, gdb)], f[np.ix_(q[gq], db[gdb])])


@pytest.mark.parametrize('shape', [(1, 4099), (4099, 1)], ids=['1x4099', '4099x1'])
def test_one_row_and_one_column_of_4099(gpu, shape):
    store, _ = C.store('one10')
    G = len(store)
    rng = np.random.default_rng(4099)
    q, db = rng.integers(0, G, size=shape[0]), rng.integers(0, G, size=shape[1])
    for budget, connected in ((100, True), (C.PROVE_BUDGET, False)):
        full = _all_pairs(gpu, 'one10', budget, connected)
        got = _run(gpu, store, budget, connected, q, db)
        _equal(got, [f[np.ix_(q, db)] for f in full])


# ---- 4. store conventions -----------------------------------------------------------------
def _copy_of(store):
    s = copy.copy(store)
    s.adj, s.types, s.n = store.adj.copy(), store.types.copy(), store.n.copy()
    s._dev = None
    return s


@pytest.mark.parametrize('what', ['weights', 'types'])
def test_edges_are_nonzero_weights_and_types_are_any_int32(gpu, what):
    """An edge is adj != 0 off the diagonal, whatever the weight and the diagonal; types are
    compared for equality only, and the root's classes are in the order of the smallest graph-1
    node, not of the type's value."""
    store, _ = C.store('four10')
    G = len(store)
    s = _copy_of(store)
    if what == 'weights':
        s.adj *= np.float32(2.5)
        d = np.arange(s.n_max)
        s.adj[:, d, d] = np.float32(1.0)                  # beyond n as well
        off = ~np.eye(s.n_max, dtype=bool)
        assert np.array_equal(s.adj[:, off] != 0, store.adj[:, off] != 0)
        edge = store.adj[:, off] != 0
        assert edge.any() and (s.adj[:, off][edge] != store.adj[:, off][edge]).all()
    else:
        ids = sorted(set(int(t) for g in range(G) for t in store.types[g, :store.n[g]]))
        assert len(ids) == 4
        to = np.array([2 ** 31 - 1, -7, -2 ** 31, 0], dtype=np.int64)   # not monotone
        lut = np.zeros(max(ids) + 1, dtype=np.int64)
        lut[ids] = to
        for g in range(G):
            n = int(store.n[g])
            s.types[g, :n] = lut[store.types[g, :n]].astype(np.int32)
        assert s.types.dtype == np.int32 and s.types.min() == -2 ** 31
        assert s.types.max() == 2 ** 31 - 1
    for budget in (7, C.PROVE_BUDGET):
        for connected in (False, True):
            _equal(_run(gpu, s, budget, connected), _all_pairs(gpu, 'four10', budget, connected))
