"""Budgeted MCS search on the GPU (include/siamese_mcs.h): size, bound, edges, map_out and
expansions_out of sg_mcs_grid equal tests/_mcs_restatement.py bit for bit at both store
capacities and both `connected` values, at budgets that cut the search off in mid-flight and at
one that proves the three small sets (test_mcs_host.py shows half of it suffices).  Then checks
that use no restatement (the map recomputed from the store arrays, the modular-product clique,
the edit path the map induces against the exact GED), position independence, entries the call
cannot serve, and the Python layer."""
import numpy as np
import pytest

import _mcs_cases as C

pytestmark = pytest.mark.gpu

CASES = [(name, b, c) for name in C.PROVEN_SETS for b in C.CUT_BUDGETS + (C.PROVE_BUDGET,)
         for c in (False, True)] + \
        [('two32', b, c) for b in C.CUT_BUDGETS + (C.LARGE_BUDGET,) for c in (False, True)]
_OUT = {}


def _run(gpu, store, budget, connected, q=None, db=None, **kw):
    """(size, bound, edges, map, expansions[, status]) as host arrays."""
    from graphembedding_amd.mcs import mcs_grid
    out = mcs_grid(store, q, db, connected=connected, budget=budget, bounds=True, edges=True,
                   mapping=True, expansions=True, device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


def _all_pairs(gpu, name, budget, connected):
    """All pairs of a set, one call per (set, budget, connected)."""
    key = (name, budget, connected)
    if key not in _OUT:
        _OUT[key] = _run(gpu, C.store(name)[0], budget, connected)
    return _OUT[key]


def _want(ref, q, db, connected, budget):
    """The restatement's grid in the order of _run."""
    size, bound, mp, ed, ex = ref.grid(q, db, connected, budget)
    return [size, bound, ed, mp, ex]


@pytest.mark.parametrize('name,budget,connected', CASES,
                         ids=['{}-{}-{}'.format(n, b, 'conn' if c else 'any') for n, b, c in CASES])
def test_all_pairs_equal_the_restatement(gpu, name, budget, connected):
    store, ref = C.store(name)
    G = len(store)
    size, bound, ed, mp, ex = _all_pairs(gpu, name, budget, connected)
    wsize, wbound, wed, wmp, wex = _want(ref, range(G), range(G), connected, budget)
    assert size.dtype == np.int32 and bound.dtype == np.int32 and ed.dtype == np.int32
    assert mp.dtype == np.int8 and ex.dtype == np.int64
    assert size.shape == bound.shape == ed.shape == ex.shape == (G, G)
    assert mp.shape == (G, G, store.n_max)
    assert np.array_equal(ex, wex), np.argwhere(ex != wex)[:5]
    assert np.array_equal(size, wsize), np.argwhere(size != wsize)[:5]
    assert np.array_equal(bound, wbound), np.argwhere(bound != wbound)[:5]
    assert np.array_equal(ed, wed), np.argwhere(ed != wed)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    assert (ex <= budget).all() and (ex >= 0).all() and (size <= bound).all()
    if budget == 0:
        assert not ex.any() and not size.any()
    if budget == C.PROVE_BUDGET:
        assert np.array_equal(size, bound) and ex.max() <= budget // 2
    if name == 'one10' and budget in (7, 100) or name == 'two32' and budget:
        assert ((ex == budget) & (size != bound)).any()        # cut off in mid-search


def _plain(store, g):
    n = int(store.n[g])
    t = [int(x) for x in store.types[g, :n]]
    E = {(a, b) for a in range(n) for b in range(n) if a != b and store.adj[g, a, b] != 0}
    return t, E


def _check_map(g1, g2, phi, connected):
    """(size, edges) of phi, a common induced subgraph (connected where asked), from the
    store's own arrays."""
    (t1, E1), (t2, E2) = g1, g2
    mapped = [a for a, b in enumerate(phi) if b >= 0]
    img = [phi[a] for a in mapped]
    assert len(set(img)) == len(img) and all(b < len(t2) for b in img)
    for a in mapped:
        assert t1[a] == t2[phi[a]]
        for c in mapped:
            assert a == c or ((a, c) in E1) == ((phi[a], phi[c]) in E2)
    if connected and mapped:
        seen, todo = set(), [mapped[0]]
        while todo:
            a = todo.pop()
            if a not in seen:
                seen.add(a)
                todo.extend(b for b in mapped if (a, b) in E1 and b not in seen)
        assert seen == set(mapped)
    return len(mapped), sum(1 for a in mapped for c in mapped if a < c and (a, c) in E1)


@pytest.mark.parametrize('name,budget', [('one10', 7), ('one10', C.PROVE_BUDGET),
                                         ('tie6', C.PROVE_BUDGET), ('four10', C.PROVE_BUDGET),
                                         ('two32', C.LARGE_BUDGET)])
def test_outputs_without_the_restatement(gpu, name, budget):
    from test_mcs_host import modular_product_clique
    store, ref = C.store(name)
    G = len(store)
    gs = [_plain(store, g) for g in range(G)]
    n_clique = 0
    for connected in (False, True):
        size, bound, ed, mp, ex = _all_pairs(gpu, name, budget, connected)
        for a in range(G):
            for b in range(G):
                n1 = len(gs[a][0])
                assert (mp[a, b, n1:] == -1).all()
                phi = [int(x) for x in mp[a, b, :n1]]
                assert _check_map(gs[a], gs[b], phi, connected) == (size[a, b], ed[a, b]), (a, b)
                if not connected and size[a, b] == bound[a, b] and \
                        max(store.n[a], store.n[b]) <= 10:
                    assert size[a, b] == modular_product_clique(ref.graph(a), ref.graph(b))
                    n_clique += 1
    assert n_clique >= {'one10': 36, 'tie6': 16, 'four10': 100, 'two32': 1}[name] or budget == 7
    if name == 'four10':
        # the edit path a common subgraph induces: delete and insert everything outside it
        from graphembedding_amd.ged import ged_grid
        ub, lb = (t.cpu().numpy() for t in ged_grid(store, bounds=True, device=gpu,
                                                    exact_budget=1 << 15))
        size, bound, ed, mp, ex = _all_pairs(gpu, name, budget, False)
        n = store.n[:G].astype(np.int64)
        e = np.array([len(g[1]) // 2 for g in gs], dtype=np.int64)
        path = n[:, None] + n[None, :] - 2 * size + e[:, None] + e[None, :] - 2 * ed
        proven = ub == lb
        assert proven.sum() > G and (ub[proven] <= path[proven]).all()
        assert not np.diag(path).any()                         # a graph against itself


def _grid_ids(shape, G):
    rng = np.random.default_rng(sum(shape))
    m, n = shape
    return rng.integers(0, G, size=m), rng.permutation(np.arange(n) % G)


@pytest.mark.parametrize('shape,ld', [((3, 5), 8), ((7, 9), 12), ((13, 11), 11)],
                         ids=['3x5', '7x9', '13x11'])
def test_grid_shapes_indices_and_ld(gpu, shape, ld):
    """Permuted and repeated ids, ld > n, pair counts (15, 63, 143) that are no multiple of the
    4 pairs of a workgroup: cheap and expensive pairs share workgroups and the last is partial."""
    store, ref = C.store('one10')
    q, db = _grid_ids(shape, len(store))
    assert (shape[0] * shape[1]) % 4
    for budget, connected in ((7, False), (100, True), (C.PROVE_BUDGET, False)):
        got = _run(gpu, store, budget, connected, q, db, ld=ld)
        want = _want(ref, q, db, connected, budget)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        again = _run(gpu, store, budget, connected, q, db, ld=ld)   # two runs: bitwise equal
        assert all(np.array_equal(g, a) for g, a in zip(got, again))
        full = _all_pairs(gpu, 'one10', budget, connected)          # equal at every position
        for g, f in zip(got, full):
            assert np.array_equal(g, f[np.ix_(q, db)])


def test_one_pair_alone_and_inside_a_grid(gpu):
    store, _ = C.store('one10')
    for budget, connected in ((100, False), (C.PROVE_BUDGET, False), (C.PROVE_BUDGET, True)):
        full = _all_pairs(gpu, 'one10', budget, connected)
        a, b = np.unravel_index(int(np.argmax(full[4])), full[4].shape)   # the costliest pair
        assert full[4][a, b] > 100 or budget == 100
        for i, j in ((a, b), (0, 6), (3, 4)):
            one = _run(gpu, store, budget, connected, [i], [j], ld=3)
            for o, f in zip(one, full):
                assert o.shape[:2] == (1, 1) and np.array_equal(o[0, 0], f[i, j]), (i, j)


def test_unservable_entries_read_minus_one_and_leave_the_rest(gpu):
    import copy

    from graphembedding_amd import _lib
    from graphembedding_amd.mcs import mcs_grid
    store, _ = C.store('one10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    budget = 100
    full = _all_pairs(gpu, 'one10', budget, False)
    q = np.array([3, -1, 6, 4, G, 5])
    db = np.array([6, 4, 3, 2 ** 31 - 1, 5, 2])
    size, bound, ed, mp, ex, status = _run(gpu, holed, budget, False, q, db, return_status=True)
    assert int(status[0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    bad_q, bad_db = [1, 3, 4], [1, 3]
    for out in (size, bound, ed, ex):
        assert (out[bad_q] == -1).all() and (out[:, bad_db] == -1).all()
    assert (mp[bad_q] == -1).all() and (mp[:, bad_db] == -1).all()
    gq, gdb = [0, 2, 5], [0, 2, 4, 5]
    for out, f in zip((size, bound, ed, mp, ex), full):       # neighbours in the same workgroup
        assert np.array_equal(out[np.ix_(gq, gdb)], f[np.ix_(q[gq], db[gdb])])
    assert (ex[np.ix_(gq, gdb)] == budget).any()
    st = lambda q_: int(_run(gpu, holed, 7, True, q_, [1], return_status=True)[5][0])  # noqa: E731
    assert st([0, G]) == _lib.SG_ERR_ARG
    assert st([0, 4]) == _lib.SG_ERR_SHAPE
    assert st([0, 3]) == 0
    with pytest.raises(_lib.SiameseHipError, match='sg_mcs_grid: SG_ERR_SHAPE'):
        mcs_grid(holed, [4], [1], device=gpu, budget=7)
    with pytest.raises(_lib.SiameseHipError, match='sg_mcs_grid: SG_ERR_ARG'):
        mcs_grid(store, [G], [1], device=gpu, budget=7)


# ---- the Python layer ---------------------------------------------------------------------
def test_mcs_matrix_pair_and_distance_mcs(gpu, monkeypatch):
    from graphembedding_amd import distance, mcs
    from graphembedding_amd.ged import csr_store_of_graphs
    graphs = C.graphs('one10')
    store, _ = C.store('one10')
    G = len(graphs)
    for connected in (False, True):
        size, bound, ed, _, _ = _all_pairs(gpu, 'one10', C.PROVE_BUDGET, connected)
        sm, proven = mcs.mcs_matrix(graphs, connected=connected, budget=C.PROVE_BUDGET,
                                    device=gpu)
        assert sm.dtype == np.int64 and proven.dtype == bool and proven.all()
        assert np.array_equal(sm, size) and np.array_equal(sm, sm.T)
        assert np.array_equal(np.diag(sm), store.n[:G])
        s7, b7, _, _, _ = _all_pairs(gpu, 'one10', 7, connected)
        sm7, proven7 = mcs.mcs_matrix(store, connected=connected, budget=7, device=gpu)
        assert np.array_equal(sm7, s7) and np.array_equal(proven7, s7 == b7)
        assert not proven7.all()
        assert mcs.mcs_pair(graphs[3], graphs[5], connected=connected, budget=C.PROVE_BUDGET,
                            device=gpu) == (size[3, 5], bound[3, 5], ed[3, 5])
        assert mcs.mcs_pair(graphs[3], graphs[5], connected=connected, budget=7,
                            device=gpu)[:2] == (s7[3, 5], b7[3, 5])
        got = distance.mcs(graphs[3], graphs[5], connected=connected)
        assert isinstance(got, int) and got == size[3, 5]
    assert distance.mcs(graphs[4], graphs[4]) == 10
    d = mcs.bunke_shearer(_all_pairs(gpu, 'one10', C.PROVE_BUDGET, False)[0], store.n[:G])
    assert d.dtype == np.float64 and not np.diag(d).any() and (d >= 0).all() and (d < 1).all()
    # the default return is the size alone; a graph store is refused
    only = mcs.mcs_grid(store, [3], [5], budget=C.PROVE_BUDGET, device=gpu)
    assert tuple(only.shape) == (1, 1) and int(only.item()) == \
        _all_pairs(gpu, 'one10', C.PROVE_BUDGET, False)[0][3, 5]
    with pytest.raises(ValueError, match='dense store only'):
        mcs.mcs_grid(csr_store_of_graphs(graphs), device=gpu)
    # an unproven pair raises with what it has: 32 nodes against 24 at a budget of 1
    big = C.graphs('two32')
    monkeypatch.setattr(mcs, 'MCS_DEFAULT_BUDGET', 1)
    with pytest.raises(RuntimeError, match=r'not proven within 1 expansions: size \d+ bound \d+'):
        distance.mcs(big[4], big[3])
