"""Device GED bounds on the GPU (include/siamese_ged.h): ub, lb and map_out of sg_ged_grid
equal tests/_ged_restatement.py bit for bit, on node counts around every lane limit of both
store capacities, on tie-heavy sets, on grids of several shapes with permuted and repeated
indices, with both_orders on and off and with entries the call cannot serve.  Three checks
use no restatement: the assignment cost recomputed from map_out and the lower bound against
scipy's LSAP optimum, and the induced cost recomputed from map_out against ub.  Then the
Python layer: ged_matrix into DistCalculator.from_matrix, distance.ged('bp'), and train.main
with the opt-in labels."""
import networkx as nx
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _ged_restatement as R

pytestmark = pytest.mark.gpu

TYPES = ('C', 'N', 'O', 'S')


def _random_graph(rng, n, gid, types=TYPES, p_extra=0.15):
    g = nx.Graph(gid=gid)
    for v in range(n):
        g.add_node(v, type=types[int(rng.integers(0, len(types)))])
    for v in range(1, n):
        g.add_edge(v, int(rng.integers(0, v)))
    for a in range(n):
        for b in range(a):
            if rng.random() < p_extra:
                g.add_edge(a, b)
    return g


def _typed(g, gid, t='C'):
    g = nx.Graph(g, gid=gid)
    nx.set_node_attributes(g, t, 'type')
    return g


def _graphs(name):
    rng = np.random.default_rng(('cap10', 'cap32', 'tie10', 'tie32').index(name) + 40)
    if name == 'cap10':     # N = n1 + n2 in {2 .. 20}
        return [_random_graph(rng, n, i) for i, n in enumerate((1, 2, 5, 9, 10, 10, 9, 5, 2, 1,
                                                                 5, 10))]
    if name == 'cap32':     # N crosses 32 and reaches the 64 lanes
        return [_random_graph(rng, n, i, p_extra=0.08)
                for i, n in enumerate((1, 15, 16, 17, 30, 32, 32, 16))]
    if name == 'tie10':     # one type; equal sizes; regular graphs: every entry of C ties
        gs = [nx.path_graph(6), nx.star_graph(5), nx.cycle_graph(6), nx.complete_graph(6)]
        gs = [_typed(g, i) for i, g in enumerate(gs)]
        return gs + [_random_graph(rng, n, 4 + i, types=('C',)) for i, n in enumerate((6, 6, 8))]
    gs = [nx.path_graph(16), nx.star_graph(15), nx.cycle_graph(16), nx.complete_graph(16),
          nx.cycle_graph(32), nx.path_graph(32)]
    return [_typed(g, i) for i, g in enumerate(gs)]


_STORES = {}


def _store(name):
    """(store, GridReference) of a named set, built once."""
    if name not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        store = store_of_graphs(_graphs(name), n_max=10 if name.endswith('10') else 32)
        _STORES[name] = (store, R.GridReference(store))
    return _STORES[name]


def _run(gpu, store, q=None, db=None, both=True, **kw):
    from graphembedding_amd.ged import ged_grid
    out = ged_grid(store, q, db, both_orders=both, bounds=True, mapping=True, device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('both', [False, True], ids=['one_order', 'both_orders'])
@pytest.mark.parametrize('name', ['cap10', 'cap32', 'tie10', 'tie32'])
def test_all_pairs_equal_the_restatement(gpu, name, both):
    store, ref = _store(name)
    G = len(store)
    ub, lb, mp = _run(gpu, store, both=both)
    wub, wlb, wmp = ref.grid(range(G), range(G), both)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert mp.shape == (G, G, store.n_max)
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    assert (lb <= ub).all() and (lb >= 0).all()
    d = np.arange(G)
    assert not ub[d, d].any() and not lb[d, d].any()          # a graph against itself
    assert np.array_equal(mp[d, d], wmp[d, d])
    if both:
        assert np.array_equal(ub, ub.T)
    assert np.array_equal(lb, lb.T)


def test_sizes_reach_every_lane_count():
    """The sets above hold what the comparison needs: N from 2 to 20 at capacity 10, N on both
    sides of 32 and N = 64 at capacity 32."""
    n10 = _store('cap10')[0].n
    assert set(n10.tolist()) == {1, 2, 5, 9, 10}
    n32 = _store('cap32')[0].n
    assert set(n32.tolist()) == {1, 15, 16, 17, 30, 32}
    sums = {int(a + b) for a in n32 for b in n32}
    assert {31, 32, 33, 64} <= sums


# grids over the capacity-10 set: permuted and repeated ids, ld > n
def _grid_ids(shape):
    rng = np.random.default_rng(sum(shape))
    G = len(_store('cap10')[0])
    m, n = shape
    if shape == (1, 1):
        return np.array([7]), np.array([3])
    return rng.integers(0, G, size=m), rng.permutation(np.arange(n) % G)


@pytest.mark.parametrize('both', [False, True], ids=['one_order', 'both_orders'])
@pytest.mark.parametrize('shape,ld', [((1, 1), 4), ((3, 5), 8), ((70, 70), 96)],
                         ids=['1x1', '3x5', '70x70'])
def test_grid_shapes_indices_and_ld(gpu, shape, ld, both):
    store, ref = _store('cap10')
    q, db = _grid_ids(shape)
    ub, lb, mp = _run(gpu, store, q, db, both=both, ld=ld)
    wub, wlb, wmp = ref.grid(q, db, both)
    assert ub.shape == shape
    assert np.array_equal(ub, wub) and np.array_equal(lb, wlb) and np.array_equal(mp, wmp)
    # ld == n gives the same values
    ub2, lb2, mp2 = _run(gpu, store, q, db, both=both)
    assert np.array_equal(ub, ub2) and np.array_equal(lb, lb2) and np.array_equal(mp, mp2)


def test_a_pair_reads_the_same_at_every_position_and_grid_size(gpu):
    """Every occurrence of an ordered pair of graphs, in the 3x5 and the 70x70 grid and in the
    all-pairs grid, gives the same ub, lb and map."""
    store, _ = _store('cap10')
    G = len(store)
    seen = {}
    n_repeats = 0
    for q, db in [(np.arange(G), np.arange(G)), _grid_ids((3, 5)), _grid_ids((70, 70))]:
        ub, lb, mp = _run(gpu, store, q, db, both=False)
        for i, a in enumerate(q):
            for j, b in enumerate(db):
                got = (int(ub[i, j]), int(lb[i, j]), mp[i, j].tobytes())
                n_repeats += (int(a), int(b)) in seen
                assert seen.setdefault((int(a), int(b)), got) == got, (a, b, i, j)
    assert n_repeats > 4000


def test_unservable_entries_read_minus_one_and_leave_the_rest(gpu):
    """A bad id and a zero node count: status is raised, that entry's pairs read -1, every
    other pair is what it is without them; no other graph is substituted."""
    import copy

    from graphembedding_amd import _lib
    store, ref = _store('cap10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    wref = R.GridReference(holed)
    wref.pairs = ref.pairs                      # the graphs that remain are unchanged
    q = np.array([0, -1, 3, 4, G, 6])
    db = np.array([5, 4, 2, 2 ** 31 - 1, 1])
    for both in (False, True):
        ub, lb, mp, status = _run(gpu, holed, q, db, both=both, return_status=True)
        wub, wlb, wmp = wref.grid(q, db, both)
        assert int(status[0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
        assert np.array_equal(ub, wub) and np.array_equal(lb, wlb) and np.array_equal(mp, wmp)
        assert (ub[[1, 3, 4]] == -1).all() and (ub[:, [1, 3]] == -1).all()
        assert (lb[[1, 3, 4]] == -1).all() and (mp[[1, 3, 4]] == -1).all()
        good = ub[np.ix_([0, 2, 5], [0, 2, 4])]
        assert (good >= 0).all()
        assert np.array_equal(good, ref.grid(q[[0, 2, 5]], db[[0, 2, 4]], both)[0])
    # each cause alone pins its code; a clean call leaves the status 0
    assert int(_run(gpu, holed, [0, G], [1], return_status=True)[3][0]) == _lib.SG_ERR_ARG
    assert int(_run(gpu, holed, [0, 4], [1], return_status=True)[3][0]) == _lib.SG_ERR_SHAPE
    assert int(_run(gpu, holed, [0, 3], [1], return_status=True)[3][0]) == 0
    from graphembedding_amd.ged import ged_grid
    with pytest.raises(_lib.SiameseHipError, match='SG_ERR_SHAPE'):
        ged_grid(holed, [4], [1], device=gpu)
    # NULL indices are graphs 0 .. m-1 / 0 .. n-1: graph 4 is among them
    ub = _run(gpu, holed, return_status=True)[0]
    assert (ub[4] == -1).all() and (ub[:, 4] == -1).all() and (np.delete(ub, 4, 0)[:, :4] >= 0).all()


# ---- without the restatement --------------------------------------------------------------
def _plain(store, g):
    """types, degrees and the edge set of store graph g, from the store's arrays alone."""
    n = int(store.n[g])
    t = [int(x) for x in store.types[g, :n]]
    E = {(a, b) for a in range(n) for b in range(n) if a != b and store.adj[g, a, b] != 0}
    deg = [sum(1 for b in range(n) if (a, b) in E) for a in range(n)]
    return t, deg, E


def _matrix(g1, g2, w):
    (t1, d1, _), (t2, d2, _) = g1, g2
    n1, n2 = len(t1), len(t2)
    C = np.full((n1 + n2, n1 + n2), 10 ** 6, dtype=np.int64)
    C[n1:, n2:] = 0
    for i in range(n1):
        for j in range(n2):
            C[i, j] = w * (t1[i] != t2[j]) + abs(d1[i] - d2[j])
        C[i, n2 + i] = w + d1[i]
    for j in range(n2):
        C[n1 + j, j] = w + d2[j]
    return C


@pytest.mark.parametrize('name', ['cap10', 'cap32', 'tie10'])
def test_map_and_bounds_against_scipy(gpu, name):
    store, _ = _store(name)
    G = len(store)
    ub, lb, mp = _run(gpu, store, both=False)
    gs = [_plain(store, g) for g in range(G)]
    for a in range(G):
        for b in range(G):
            (t1, d1, E1), (t2, d2, E2) = gs[a], gs[b]
            n1, n2 = len(t1), len(t2)
            phi = [int(x) for x in mp[a, b, :n1]]
            kept = [x for x in phi if x >= 0]
            assert len(set(kept)) == len(kept) and all(x < n2 for x in kept)
            assert (mp[a, b, n1:] == -1).all()
            # the assignment cost of phi on the upper-bound matrix is the LSAP optimum
            C = _matrix(gs[a], gs[b], 1)
            r, c = linear_sum_assignment(C)
            cost = sum(C[i, phi[i]] if phi[i] >= 0 else C[i, n2 + i] for i in range(n1))
            cost += sum(C[n1 + j, j] for j in range(n2) if j not in kept)
            assert cost == C[r, c].sum(), (a, b)
            # the edit path phi induces costs ub
            dels = n1 - len(kept)
            subs = sum(1 for i in range(n1) if phi[i] >= 0 and t1[i] != t2[phi[i]])
            both_e = sum(1 for (x, y) in E1 if phi[x] >= 0 and phi[y] >= 0 and
                         (phi[x], phi[y]) in E2)       # ordered pairs: every edge twice
            induced = dels + (n2 - len(kept)) + subs + (len(E1) + len(E2)) // 2 - both_e
            assert induced == ub[a, b], (a, b)
            # the lower bound is half the optimum of the half-edge-cost matrix, rounded up
            C2 = _matrix(gs[a], gs[b], 2)
            r, c = linear_sum_assignment(C2)
            assert lb[a, b] == -(-int(C2[r, c].sum()) // 2), (a, b)


# ---- the Python layer ---------------------------------------------------------------------
def test_ged_matrix_feeds_dist_calculator_and_distance_ged(gpu):
    from graphembedding_amd import distance
    from graphembedding_amd.dist_calculator import DistCalculator
    from graphembedding_amd.ged import ged_matrix
    graphs = _graphs('cap10')
    store, ref = _store('cap10')
    G = len(graphs)
    dm = ged_matrix(graphs, device=gpu)
    assert dm.dtype == np.int64 and dm.shape == (G, G)
    assert np.array_equal(dm, dm.T) and not np.diag(dm).any()
    assert np.array_equal(dm, ref.grid(range(G), range(G), True)[0])
    assert np.array_equal(dm, ged_matrix(store, device=gpu))
    dc = DistCalculator.from_matrix('none', graphs, dm, 'ged', 'bp')
    d, dn = dc.calculate_dist(graphs[3], graphs[5])
    assert d == dm[3, 5] and dn == 2 * d / (9 + 10)
    assert distance.ged(graphs[3], graphs[5], 'bp') == dm[3, 5]
    assert distance.ged(graphs[0], graphs[0], 'bp') == 0
    # a miss of the map computes through distance.ged
    fresh = DistCalculator('none', 'ged', 'bp', gidpair_dist_map={})
    assert fresh.calculate_dist(graphs[2], graphs[4])[0] == dm[2, 4]


def test_load_graph_set_with_bp_labels(gpu):
    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.ged import ged_grid
    gs = load_graph_set('syn_aids80nef', ged='bp', device=gpu)
    ub, lb = (t.cpu().numpy() for t in ged_grid(gs.store, bounds=True, device=gpu))
    assert gs.ged.dtype == np.int64 and np.array_equal(gs.ged, ub)
    assert np.array_equal(ub, ub.T) and not np.diag(ub).any() and (lb <= ub).all()
    ref = R.GridReference(gs.store)
    q, db = np.arange(0, 80, 9), np.arange(3, 80, 11)
    wub, wlb, _ = ref.grid(q, db, True)
    assert np.array_equal(ub[np.ix_(q, db)], wub) and np.array_equal(lb[np.ix_(q, db)], wlb)
    lab = gs.label_matrix(0.6)
    assert lab.shape == (80, 80) and np.isfinite(lab).all() and (np.diag(lab) == 1).all()


def test_train_main_with_bp_labels(gpu):
    """main() with ged_labels='bp' runs its 20 default iterations on syn_aids700nef to a finite
    loss; with the default the label matrix is the synthetic one, as before."""
    from graphembedding_amd.config import Flags
    from graphembedding_amd.data import synthetic_ged_matrix
    from graphembedding_amd.ged import ged_matrix
    from graphembedding_amd.train import main
    kw = dict(dataset='syn_aids700nef', n_max=10, node_feat_order='sorted', test_path='embed')
    f = Flags(ged_labels='bp', **kw)
    assert f.iters == 20
    tr, _, (data, dc, _) = main(f, device=gpu, return_objects=True)
    idx, dm = dc.matrix
    by_gid = {g.graph['gid']: g for g in list(data.orig_train_graphs) +
              [data.test_data.gs[i].nxgraph for i in range(data.m)]}
    gs = [by_gid[k] for k in sorted(idx, key=idx.get)]
    assert dm.shape == (700, 700) and np.array_equal(dm, ged_matrix(gs, device=gpu))
    assert not np.array_equal(dm, synthetic_ged_matrix(gs))
    losses = np.asarray(tr[0], dtype=np.float64)
    assert losses.size == 20 and np.isfinite(losses).all()
    f0 = Flags(iters=1, **dict(kw, dataset='syn_aids80nef'))
    assert f0.ged_labels == 'synthetic'
    _, _, (data0, dc0, _) = main(f0, device=gpu, return_objects=True)
    idx0, dm0 = dc0.matrix
    by_gid = {g.graph['gid']: g for g in list(data0.orig_train_graphs) +
              [data0.test_data.gs[i].nxgraph for i in range(data0.m)]}
    assert np.array_equal(dm0, synthetic_ged_matrix([by_gid[k] for k in sorted(idx0, key=idx0.get)]))
