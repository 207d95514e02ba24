"""Both GED kernels on the graph classes of tests/_ged_classes.py (edgeless, disconnected, dense,
29 types, planted pairs up to 16 nodes): bit for bit against the restatements at budgets that
cut the search and at one that proves every within-set pair (test_ged_classes_host.py shows
half of it suffices), and against the closed forms, planted bounds, metric axioms and networkx,
which need no restatement.  Then store capacities 1, 2, 16, 17 and 31 against capacity 32,
a store with a unit diagonal and scaled weights, and the Python layer."""
import copy

import networkx as nx
import numpy as np
import pytest

import _ged_classes as K
import _ged_exact_restatement as X
import _ged_restatement as R

pytestmark = pytest.mark.gpu

_BP, _EX = {}, {}


@pytest.fixture(scope='module')
def cache(request, tmp_path_factory):
    if hasattr(request.config, 'cache') and request.config.cache is not None:
        return request.config.cache.mkdir('ged_classes')
    return tmp_path_factory.mktemp('ged_classes')


def _bp(gpu, name, both):
    from graphembedding_amd.ged import ged_grid
    if (name, both) not in _BP:
        out = ged_grid(K.store(name)[0], both_orders=both, bounds=True, mapping=True, device=gpu)
        _BP[(name, both)] = [t.cpu().numpy() for t in out]
    return _BP[(name, both)]


def _exact(gpu, store, budget, **kw):
    from graphembedding_amd.ged import ged_grid
    out = ged_grid(store, bounds=True, mapping=True, expansions=True, exact_budget=budget,
                   device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


def _ex(gpu, name, budget):
    if (name, budget) not in _EX:
        _EX[(name, budget)] = _exact(gpu, K.store(name)[0], budget)
    return _EX[(name, budget)]


def _plain(store, g):
    n = int(store.n[g])
    t = [int(x) for x in store.types[g, :n]]
    E = {(a, b) for a in range(n) for b in range(n) if a != b and store.adj[g, a, b] != 0}
    return t, E


def _induced(g1, g2, phi):
    """test_gpu_ged_exact.py's."""
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


def _check_maps(store, mp, ub):
    G = len(store)
    gs = [_plain(store, g) for g in range(G)]
    for a in range(G):
        for b in range(G):
            n1 = len(gs[a][0])
            assert (mp[a, b, n1:] == -1).all()
            assert _induced(gs[a], gs[b], [int(x) for x in mp[a, b, :n1]]) == ub[a, b], (a, b)


# ---- 1. the bipartite call --------------------------------------------------------------------
@pytest.mark.parametrize('both', [False, True], ids=['one_order', 'both_orders'])
@pytest.mark.parametrize('name', K.SETS)
def test_bipartite_call_on_every_set(gpu, name, both):
    store, ref, _ = K.store(name)
    G = len(store)
    ub, lb, mp = _bp(gpu, name, both)
    wub, wlb, wmp = ref.grid(range(G), range(G), both)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert mp.shape == (G, G, store.n_max)
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    for (a, b), (kind, v) in K.known(name).items():
        assert lb[a, b] <= v, (a, b, lb[a, b], v)
        assert kind == 'le' or v <= ub[a, b], (a, b, v, ub[a, b])
    if not both:                                 # map is the 1->2 order's: it induces that ub
        _check_maps(store, mp, ub)
    if name == 'edge0':
        assert np.array_equal(ub, lb)


# ---- 2. the exact call ------------------------------------------------------------------------
EXACT = [(name, b) for name in K.SETS for b in K.CUT_BUDGETS + (K.PROVE_BUDGET_WIDE,)]


@pytest.mark.parametrize('name,budget', EXACT, ids=['{}-{}'.format(*c) for c in EXACT])
def test_exact_call_on_every_set(gpu, name, budget, cache):
    store, _, ref = K.store(name)
    G = len(store)
    ub, lb, mp, ex = _ex(gpu, name, budget)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert ex.dtype == np.int64 and mp.shape == (G, G, store.n_max)
    if budget == K.PROVE_BUDGET_WIDE:
        # every within-set search ends within half of it (test_ged_classes_host.py), so the
        # unlimited restatement is the restatement at this budget
        solved = K.solved(name, cache)
        wub, wlb, wmp, wex = ref.grid(range(G), range(G), 0)
        for (a, b), (u, l, phi, e) in solved.items():
            assert e <= budget // 2
            wub[a, b], wlb[a, b], wex[a, b] = u, l, e
            wmp[a, b] = -1
            wmp[a, b, :len(phi)] = phi
    else:
        wub, wlb, wmp, wex = ref.grid(range(G), range(G), budget)
    assert np.array_equal(ex, wex), np.argwhere(ex != wex)[:5]
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    assert (ex <= budget).all() and (ex >= 0).all() and (lb <= ub).all()
    n = store.n
    big = np.maximum(n[:, None], n[None, :]) > X.MAX_SEARCH_NODES
    assert not ex[big].any()
    _check_maps(store, mp, ub)
    ub0, lb0, _ = _bp(gpu, name, True)
    assert (ub <= ub0).all() and (lb >= lb0).all()
    assert np.array_equal(lb[ub != lb], lb0[ub != lb])
    for (a, b), (kind, v) in K.known(name).items():            # lb <= known <= ub at any budget
        assert lb[a, b] <= v and (kind == 'le' or v <= ub[a, b]), (a, b)
    if name == 'edge0':
        assert not ex.any() and np.array_equal(ub, lb)         # the assignment is exact there


@pytest.mark.parametrize('name', K.SETS)
def test_proven_distances_without_the_restatement(gpu, name):
    """At PROVE_BUDGET_WIDE: every searched pair is proven, and the proven distances are the
    closed forms, 0 by an isomorphism on (g, pi(g)), within the planted bounds, a metric, and
    networkx's on the small pairs."""
    store = K.store(name)[0]
    gs = K.graphs(name)
    G = len(gs)
    ub, lb, mp, ex = _ex(gpu, name, K.PROVE_BUDGET_WIDE)
    proven = ub == lb
    for a, b in K.searched_pairs(name):
        assert proven[a, b], (a, b, ub[a, b], lb[a, b], ex[a, b])
    assert ex.max() <= K.PROVE_BUDGET_WIDE // 2
    known = K.known(name)
    for (a, b), rule in known.items():
        if proven[a, b]:
            assert K.holds(rule, int(ub[a, b])), (a, b, ub[a, b], rule)
            if rule == ('eq', 0):
                assert K.is_isomorphism(gs[a], gs[b], mp[a, b]), (a, b)
    if name in K.PLANTED:
        assert ub[0, 1] == 0 and ub[1, 0] == 0 and len(known) == G * G
    d = np.arange(G)
    assert proven[d, d].all() and not ub[d, d].any()
    both = proven & proven.T
    assert np.array_equal(ub[both], ub.T[both])
    for i in range(G):
        for j in range(G):
            for k in range(G):
                if proven[i, j] and proven[i, k] and proven[k, j]:
                    assert ub[i, j] <= ub[i, k] + ub[k, j], (i, j, k)
    n_nx = 0
    for a in range(G):
        for b in range(G):
            if proven[a, b] and max(store.n[a], store.n[b]) <= 6:
                assert ub[a, b] == _nx_ged(gs[a], gs[b]), (a, b)
                n_nx += 1
    assert n_nx >= {'edge0': 9, 'forest': 4, 'types29': 4}.get(name, 1 if name in K.DENSE else 0)


# ---- 3. reach ---------------------------------------------------------------------------------
def test_the_proven_pairs_reach_sixteen_nodes(gpu):
    results, bp = {}, {}
    for name in K.SETS:
        ub, lb, mp, ex = _ex(gpu, name, K.PROVE_BUDGET_WIDE)
        ub0 = _bp(gpu, name, True)[0]
        pairs = K.searched_pairs(name)
        results[name] = {(a, b): (int(ub[a, b]), int(lb[a, b]), mp[a, b], int(ex[a, b]))
                         for a, b in pairs}
        bp[name] = {(a, b): int(ub0[a, b]) for a, b in pairs}
    for what, pairs in K.reach(results, bp).items():
        print(what, pairs[:3])
        assert pairs, what


# ---- 4. capacities ----------------------------------------------------------------------------
def _capacity_graphs(c):
    """Graphs of 1 .. c nodes: first nodes of types29's largest graph and of the forests,
    edgeless ones above 16 nodes, and one of exactly c nodes."""
    t29, fo, e0 = K.graphs('types29'), K.graphs('forest'), K.graphs('edge0')
    pool = [g for g in t29 + fo if g.number_of_nodes() <= c]
    sizes = sorted({1, min(2, c), c // 2 or 1, c})
    out = []
    for s in sizes:
        src = t29[-1] if s <= 16 else e0[-1]
        g = nx.Graph(src.subgraph(range(s)))
        out.append(g)
    out += pool[-3:] + ([e0[6]] if c >= 17 else [])
    return [nx.Graph(g, gid=i) for i, g in enumerate(out)]


def _raw(gpu, store, budget, q, db, ld):
    """Both calls through _lib on buffers filled beforehand: (ub, lb, map, expansions) as
    [m][ld] / [m][n][n_max] host arrays, the padding columns included."""
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.ged import _index
    dev_store = store.to_device(gpu)
    dev = dev_store[0].device
    m, n, nm = len(q), len(db), store.n_max
    qd, dbd = _index(q, dev), _index(db, dev)
    fill = -77
    ub = torch.full((m, ld), fill, dtype=torch.int32, device=dev)
    lb = torch.full((m, ld), fill, dtype=torch.int32, device=dev)
    mp = torch.full((m, n, nm), fill, dtype=torch.int8, device=dev)
    ex = torch.full((m, ld), fill, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if budget is None:
        ws = torch.empty(_lib.ged_grid_workspace_bytes(m, n, nm) // 4 + 1, dtype=torch.int32,
                         device=dev)
        _lib.ged_grid(dev_store, nm, qd, m, dbd, n, True, ub, ld, lb, mp, status, ws)
    else:
        ws = torch.empty(_lib.ged_exact_grid_workspace_bytes(m, n, nm) // 4 + 1,
                         dtype=torch.int32, device=dev)
        _lib.ged_exact_grid(dev_store, nm, qd, m, dbd, n, budget, ub, ld, lb, mp, ex, status, ws)
    assert int(status.item()) == 0
    out = [t.cpu().numpy() for t in (ub, lb, mp, ex)]
    for t in (out[0], out[1]) + ((out[3],) if budget is not None else ()):
        assert (t[:, n:] == fill).all() and (t[:, :n] != fill).all()      # padding untouched
    return out


@pytest.mark.parametrize('c', [1, 2, 16, 17, 31])
def test_store_capacities_against_capacity_32(gpu, c):
    from graphembedding_amd.ged import store_of_graphs
    gs = _capacity_graphs(c)
    n = [g.number_of_nodes() for g in gs]
    assert min(n) == 1 and max(n) == c
    small, wide = store_of_graphs(gs, n_max=c), store_of_graphs(gs, n_max=32)
    assert small.n_max == c and np.array_equal(small.types[:, :c], wide.types[:, :c])
    G = len(gs)
    m, nd = next((m, nd) for m in (G, G + 1) for nd in (G, G + 1, G + 2) if (m * nd) % 4)
    q, db = np.arange(m) % G, (np.arange(nd)[::-1] * 5 + 1) % G
    ld = len(db) + 3
    bref, xref = R.GridReference(small), X.ExactGridReference(small)
    for budget in (None, 1000, 7):
        got = _raw(gpu, small, budget, q, db, ld)
        ref = _raw(gpu, wide, budget, q, db, ld)
        assert got[2].shape == (len(q), len(db), c)
        for k in (0, 1, 3):
            assert np.array_equal(got[k], ref[k]), (budget, k)
        assert np.array_equal(got[2], ref[2][:, :, :c])
        assert (ref[2][:, :, c:] == -1).all()
        for i, a in enumerate(q):
            assert (got[2][i, :, n[a]:] == -1).all()
        want = bref.grid(q, db, True) if budget is None else xref.grid(q, db, budget)
        nd = len(db)
        assert np.array_equal(got[0][:, :nd], want[0]) and np.array_equal(got[1][:, :nd], want[1])
        assert np.array_equal(got[2], want[2])
        if budget is not None:
            ex = got[3][:, :nd]
            assert np.array_equal(ex, want[3])
            nq, ndb = np.asarray(n)[q], np.asarray(n)[db]
            big = np.maximum(nq[:, None], ndb[None, :]) > 16
            assert not ex[big].any() and big.any() == (c > 16)
            assert c < 16 or ex.any()


# ---- 5. diagonal and weights ------------------------------------------------------------------
def test_diagonal_and_weights_of_the_store_do_not_matter(gpu):
    from graphembedding_amd.ged import ged_grid, store_of_graphs
    gs = [g for g in K.graphs('types29') + K.graphs('forest') if g.number_of_nodes() <= 10]
    plain = store_of_graphs(gs, n_max=10)
    eye = np.eye(10, dtype=bool)[None]
    scaled, binary = copy.copy(plain), copy.copy(plain)
    scaled.adj = np.where(eye, np.float32(1.0), plain.adj * np.float32(2.5)).astype(np.float32)
    binary.adj = np.where(eye, np.float32(0.0), (plain.adj != 0).astype(np.float32))
    variants = [scaled, binary]
    for s in variants:
        s._dev = None
        assert np.array_equal((s.adj != 0) & ~eye, (plain.adj != 0) & ~eye)
    assert (plain.adj[0, 0, 0] not in (0.0, 1.0)) and plain.adj[0, 9, 9] == 0.0   # A-hat itself
    want_bp = [t.cpu().numpy() for t in ged_grid(plain, bounds=True, mapping=True, device=gpu)]
    want_ex = {b: _exact(gpu, plain, b) for b in (7, 1000)}
    assert want_ex[1000][3].any()
    for s in variants:
        got = [t.cpu().numpy() for t in ged_grid(s, bounds=True, mapping=True, device=gpu)]
        assert all(np.array_equal(g, w) for g, w in zip(got, want_bp))
        for b in (7, 1000):
            assert all(np.array_equal(g, w) for g, w in zip(_exact(gpu, s, b), want_ex[b]))


# ---- 6. the Python layer ----------------------------------------------------------------------
def test_ged_matrix_proves_a_planted_set(gpu):
    from graphembedding_amd import ged
    gs = K.graphs('planted15')
    dm, proven = ged.ged_matrix(gs, device=gpu, exact_budget=K.PROVE_BUDGET_WIDE)
    assert proven.all() and np.array_equal(dm, dm.T)
    zero = np.eye(len(gs), dtype=bool)
    zero[0, 1] = zero[1, 0] = True
    assert np.array_equal(dm == 0, zero)
    cost = np.asarray(K.PLANTED_COST)
    assert (dm <= np.abs(cost[:, None] - cost[None, :])).all()
