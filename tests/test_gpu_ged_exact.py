"""Budgeted exact GED on the GPU (include/siamese_ged_exact.h): ub, lb, map_out and
expansions_out of sg_ged_exact_grid equal tests/_ged_exact_restatement.py bit for bit at both
store capacities, at budgets that cut the search off in mid-flight and at one that proves the
whole capacity-10 set (test_ged_exact_host.py shows half of it suffices).  Then checks that use
no restatement (the induced cost of map_out, the bipartite call's bounds, metric axioms on the
proven pairs, networkx on the small ones), position independence, entries the call cannot
serve, and the Python layer."""
import networkx as nx
import numpy as np
import pytest

import _ged_exact_cases as C

pytestmark = pytest.mark.gpu

CASES = [(name, b) for name in ('cap10', 'tie10') for b in C.CUT_BUDGETS + (C.PROVE_BUDGET,)] + \
        [('cap32', b) for b in C.CUT_BUDGETS]
_OUT = {}


def _run(gpu, store, budget, q=None, db=None, **kw):
    from graphembedding_amd.ged import ged_grid
    out = ged_grid(store, q, db, bounds=True, mapping=True, expansions=True, exact_budget=budget,
                   device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


def _all_pairs(gpu, name, budget):
    """(ub, lb, map, expansions) of all pairs of a set, one call per (set, budget)."""
    if (name, budget) not in _OUT:
        _OUT[(name, budget)] = _run(gpu, C.store(name)[0], budget)
    return _OUT[(name, budget)]


@pytest.mark.parametrize('name,budget', CASES, ids=['{}-{}'.format(*c) for c in CASES])
def test_all_pairs_equal_the_restatement(gpu, name, budget):
    store, ref = C.store(name)
    G = len(store)
    ub, lb, mp, ex = _all_pairs(gpu, name, budget)
    wub, wlb, wmp, wex = ref.grid(range(G), range(G), budget)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert ex.dtype == np.int64 and mp.shape == (G, G, store.n_max)
    assert np.array_equal(ex, wex), np.argwhere(ex != wex)[:5]
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    assert (ex <= budget).all() and (ex >= 0).all()
    n = store.n
    if budget == 0:
        assert not ex.any()
    if budget == C.PROVE_BUDGET:
        assert np.array_equal(ub, lb) and ex.max() <= budget // 2 and ex.max() > 1000
    if name == 'cap32':                       # the search limit: 16 nodes searched, 17 not
        big = np.maximum(n[:, None], n[None, :]) > 16
        assert not ex[big].any() and big.any()
        if budget:
            i16, i15 = list(n).index(16), list(n).index(15)
            assert ex[i16, i15] == budget and ex[i15, i16] == budget and ex[i16, i16] == 0
    if budget in (7, 1000):                   # cut off in mid-search somewhere
        assert (ex == budget).any() and (ub != lb).any()


def _plain(store, g):
    n = int(store.n[g])
    t = [int(x) for x in store.types[g, :n]]
    E = {(a, b) for a in range(n) for b in range(n) if a != b and store.adj[g, a, b] != 0}
    return t, E


def _induced(g1, g2, phi):
    (t1, E1), (t2, E2) = g1, g2
    kept = [x for x in phi if x >= 0]
    assert len(set(kept)) == len(kept) and all(x < len(t2) for x in kept)
    subs = sum(1 for a, x in enumerate(phi) if x >= 0 and t1[a] != t2[x])
    both = sum(1 for (a, b) in E1 if phi[a] >= 0 and phi[b] >= 0 and (phi[a], phi[b]) in E2)
    return (len(t1) - len(kept)) + (len(t2) - len(kept)) + subs + (len(E1) + len(E2)) // 2 - both


def _nx_ged(g1, g2):
    d = nx.graph_edit_distance(g1, g2, node_match=lambda a, b: a['type'] == b['type'])
    assert d == int(d)
    return int(d)


@pytest.mark.parametrize('name,budget', [('cap10', 7), ('cap10', C.PROVE_BUDGET),
                                         ('tie10', C.PROVE_BUDGET), ('cap32', 1000)])
def test_outputs_without_the_restatement(gpu, name, budget):
    from graphembedding_amd.ged import ged_grid
    store, _ = C.store(name)
    G = len(store)
    ub, lb, mp, ex = _all_pairs(gpu, name, budget)
    ub0, lb0 = (t.cpu().numpy() for t in ged_grid(store, bounds=True, device=gpu))
    assert (lb <= ub).all() and (ub <= ub0).all() and (lb >= lb0).all()
    assert np.array_equal(lb[ub != lb], lb0[ub != lb])          # unproven: the bipartite lb
    gs = [_plain(store, g) for g in range(G)]
    for a in range(G):
        for b in range(G):
            n1 = len(gs[a][0])
            assert (mp[a, b, n1:] == -1).all()
            assert _induced(gs[a], gs[b], [int(x) for x in mp[a, b, :n1]]) == ub[a, b], (a, b)
    # the costs are a metric: on the proven pairs d is symmetric, zero on the diagonal, and
    # every proven triple satisfies the triangle inequality
    proven = ub == lb
    d = np.arange(G)
    assert proven[d, d].all() and not ub[d, d].any()
    both = proven & proven.T
    assert np.array_equal(ub[both], ub.T[both])
    for i in range(G):
        for j in range(G):
            for k in range(G):
                if proven[i, j] and proven[i, k] and proven[k, j]:
                    assert ub[i, j] <= ub[i, k] + ub[k, j], (i, j, k)
    # proven pairs of graphs of at most 6 nodes equal networkx
    graphs = C.graphs(name)
    n_checked = 0
    for a in range(G):
        for b in range(a, G):
            if proven[a, b] and max(store.n[a], store.n[b]) <= 6:
                assert ub[a, b] == _nx_ged(graphs[a], graphs[b]), (a, b)
                n_checked += 1
    assert n_checked >= {'cap10': 15, 'tie10': 10, 'cap32': 1}[name] or budget == 7


def _grid_ids(shape):
    rng = np.random.default_rng(sum(shape))
    G = len(C.store('cap10')[0])
    m, n = shape
    return rng.integers(0, G, size=m), rng.permutation(np.arange(n) % G)


@pytest.mark.parametrize('shape,ld', [((3, 5), 8), ((7, 9), 12), ((13, 11), 11)],
                         ids=['3x5', '7x9', '13x11'])
def test_grid_shapes_indices_and_ld(gpu, shape, ld):
    """Permuted and repeated ids, ld > n, pair counts (15, 63, 143) that are no multiple of the
    4 pairs of a workgroup: cheap and expensive pairs share workgroups and the last is partial."""
    store, ref = C.store('cap10')
    q, db = _grid_ids(shape)
    assert (shape[0] * shape[1]) % 4
    for budget in (7, C.PROVE_BUDGET):
        got = _run(gpu, store, budget, q, db, ld=ld)
        want = ref.grid(q, db, budget)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        again = _run(gpu, store, budget, q, db, ld=ld)             # two runs: bitwise equal
        assert all(np.array_equal(g, a) for g, a in zip(got, again))
        full = _all_pairs(gpu, 'cap10', budget)                    # and equal at every position
        for g, f in zip(got, full):
            assert np.array_equal(g, f[np.ix_(q, db)])


def test_one_pair_alone_and_inside_a_grid(gpu):
    store, _ = C.store('cap10')
    for budget in (1000, C.PROVE_BUDGET):
        full = _all_pairs(gpu, 'cap10', budget)
        a, b = np.unravel_index(int(np.argmax(full[3])), full[3].shape)   # the costliest pair
        assert full[3][a, b] > 1000 or budget == 1000
        for i, j in ((a, b), (0, 9), (3, 4)):
            one = _run(gpu, store, budget, [i], [j], ld=3)
            for o, f in zip(one, full):
                assert o.shape[:2] == (1, 1) and np.array_equal(o[0, 0], f[i, j]), (i, j)


def test_unservable_entries_read_minus_one_and_leave_the_rest(gpu):
    import copy

    from graphembedding_amd import _lib
    from graphembedding_amd.ged import ged_grid
    store, _ = C.store('cap10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    budget = 1000
    full = _all_pairs(gpu, 'cap10', budget)
    q = np.array([3, -1, 7, 4, G, 6])
    db = np.array([9, 4, 3, 2 ** 31 - 1, 7, 5])
    ub, lb, mp, ex, status = _run(gpu, holed, budget, q, db, return_status=True)
    assert int(status[0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    bad_q, bad_db = [1, 3, 4], [1, 3]
    for out in (ub, lb, ex):
        assert (out[bad_q] == -1).all() and (out[:, bad_db] == -1).all()
    assert (mp[bad_q] == -1).all() and (mp[:, bad_db] == -1).all()
    gq, gdb = [0, 2, 5], [0, 2, 4, 5]
    for out, f in zip((ub, lb, mp, ex), full):                # neighbours in the same workgroup
        assert np.array_equal(out[np.ix_(gq, gdb)], f[np.ix_(q[gq], db[gdb])])
    assert (ex[np.ix_(gq, gdb)] > 0).any()
    assert int(_run(gpu, holed, 7, [0, G], [1], return_status=True)[4][0]) == _lib.SG_ERR_ARG
    assert int(_run(gpu, holed, 7, [0, 4], [1], return_status=True)[4][0]) == _lib.SG_ERR_SHAPE
    assert int(_run(gpu, holed, 7, [0, 3], [1], return_status=True)[4][0]) == 0
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_exact_grid: SG_ERR_SHAPE'):
        ged_grid(holed, [4], [1], device=gpu, exact_budget=7)


# ---- the Python layer ---------------------------------------------------------------------
def test_ged_matrix_pair_and_distance_ged(gpu, monkeypatch):
    from graphembedding_amd import distance, ged
    from graphembedding_amd.dist_calculator import DistCalculator
    graphs = C.graphs('cap10')
    store, _ = C.store('cap10')
    G = len(graphs)
    ub, lb, _, _ = _all_pairs(gpu, 'cap10', C.PROVE_BUDGET)
    dm, proven = ged.ged_matrix(graphs, device=gpu, exact_budget=C.PROVE_BUDGET)
    assert dm.dtype == np.int64 and proven.dtype == bool and proven.all()
    assert np.array_equal(dm, ub) and np.array_equal(dm, dm.T) and not np.diag(dm).any()
    dm7, proven7 = ged.ged_matrix(store, device=gpu, exact_budget=7)
    ub7, lb7, _, _ = _all_pairs(gpu, 'cap10', 7)
    assert np.array_equal(dm7, ub7) and np.array_equal(proven7, ub7 == lb7) and not proven7.all()
    assert np.array_equal(ged.ged_matrix(store, device=gpu), ged.ged_matrix(graphs, device=gpu))
    dc = DistCalculator.from_matrix('none', graphs, dm, 'ged', 'exact')
    d, dn = dc.calculate_dist(graphs[3], graphs[5])
    assert d == dm[3, 5] and dn == 2 * d / (8 + 7)
    assert ged.ged_pair(graphs[3], graphs[5], device=gpu, exact_budget=7) == (ub7[3, 5], lb7[3, 5])
    assert ged.ged_pair(graphs[3], graphs[5], device=gpu)[0] >= dm[3, 5]
    assert distance.ged(graphs[3], graphs[5], 'exact') == dm[3, 5]
    assert distance.ged(graphs[0], graphs[0], 'exact') == 0
    fresh = DistCalculator('none', 'ged', 'exact', gidpair_dist_map={})
    assert fresh.calculate_dist(graphs[2], graphs[6])[0] == dm[2, 6]
    # an unproven pair raises with its bounds: 16 nodes against 15 at a budget of 1
    big = C.graphs('cap32')
    monkeypatch.setattr(ged, 'GED_EXACT_DEFAULT_BUDGET', 1)
    with pytest.raises(RuntimeError, match=r'not proven within 1 expansions: ub \d+ lb \d+'):
        distance.ged(big[3], big[2], 'exact')
    with pytest.raises(ValueError, match='exact_budget'):
        ged.ged_grid(store, expansions=True, device=gpu)


def test_load_graph_set_and_train_main_with_exact_labels(gpu, caplog):
    import logging

    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.config import Flags
    from graphembedding_amd.ged import GED_EXACT_DEFAULT_BUDGET, ged_grid, ged_matrix
    from graphembedding_amd.train import main
    with caplog.at_level(logging.INFO, logger='graphembedding_amd.ged'):
        gs = load_graph_set('syn_aids80nef', ged='exact', device=gpu)
    assert 'of 6400 pairs left unproven' in caplog.text
    ub, lb = (t.cpu().numpy() for t in ged_grid(gs.store, bounds=True, device=gpu))
    assert gs.ged.dtype == np.int64 and gs.ged.shape == (80, 80)
    assert (gs.ged <= ub).all() and (gs.ged >= lb).all() and (gs.ged < ub).any()
    assert np.array_equal(gs.ged, gs.ged.T) and not np.diag(gs.ged).any()
    f = Flags(ged_labels='exact', iters=3, dataset='syn_aids80nef', n_max=10,
              node_feat_order='sorted', test_path='embed')
    tr, _, (data, dc, _) = main(f, device=gpu, return_objects=True)
    idx, dm = dc.matrix
    by_gid = {g.graph['gid']: g for g in list(data.orig_train_graphs) +
              [data.test_data.gs[i].nxgraph for i in range(data.m)]}
    graphs = [by_gid[k] for k in sorted(idx, key=idx.get)]
    want, proven = ged_matrix(graphs, device=gpu, exact_budget=GED_EXACT_DEFAULT_BUDGET)
    assert dm.shape == (80, 80) and np.array_equal(dm, want)
    print('syn_aids80nef: {} of 6400 pairs proven'.format(int(proven.sum())))
    losses = np.asarray(tr[0], dtype=np.float64)
    assert losses.size == 3 and np.isfinite(losses).all()
