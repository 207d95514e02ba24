"""GED refinement on the GPU (include/siamese_ged_refine.h): ub, lb, map_out and moves_out of
sg_ged_refine_grid equal tests/_ged_refine_restatement.py bit for bit on every grid and budget
of _ged_refine_cases.py (test_ged_refine_host.py shows what those grids hold: every kind of move
the seeds allow, both starts winning, the partial, exact and just-over rounds of 64 lanes and
the full 16).  Then checks that use no restatement (the induced cost of map_out, the bipartite
call's bounds), grid layout and position independence, entries the call cannot serve, a grid of
many repeated ids, and the Python layer."""
import numpy as np
import pytest

import _ged_refine_cases as RC
import _ged_refine_restatement as F

pytestmark = pytest.mark.gpu

CASES = [(name, k, q, db) for name, budgets, q, db in RC.GRIDS for k in budgets]
_OUT = {}


def _run(gpu, store, budget, q=None, db=None, **kw):
    from graphembedding_amd.ged import ged_grid
    out = ged_grid(store, q, db, bounds=True, mapping=True, moves=True, refine_moves=budget,
                   device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


def _grid(gpu, name, budget, q=None, db=None):
    """(ub, lb, map, moves) of a grid of a set, one call per (set, budget, grid)."""
    key = (name, budget, q, db)
    if key not in _OUT:
        _OUT[key] = _run(gpu, RC.store(name)[0], budget, q, db)
    return _OUT[key]


@pytest.mark.parametrize('name,budget,q,db', CASES,
                         ids=['{}-k{}'.format(c[0], c[1]) for c in CASES])
def test_grids_equal_the_restatement(gpu, name, budget, q, db):
    store, ref = RC.store(name)
    ub, lb, mp, mv = _grid(gpu, name, budget, q, db)
    qi, dbi = RC.ids(name, q), RC.ids(name, db)
    wub, wlb, wmp, wmv = ref.grid(qi, dbi, budget)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert mv.dtype == np.int32 and mp.shape == (len(qi), len(dbi), store.n_max)
    assert np.array_equal(mv, wmv), np.argwhere(mv != wmv)[:5]
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    assert (mv >= 0).all() and (mv <= 2 * budget).all()
    if budget == 0:
        assert not mv.any()
    else:
        assert (mv > 0).any() and (ub != lb).any()


def test_the_rounds_of_64_lanes(gpu):
    """The pairs of 1, 63, 64, 65 and 1024 moves, each alone in a 1 x 1 grid and in both orders."""
    store, ref = RC.store('r32')
    for k, (a, b) in sorted(RC.ROUNDS.items()):
        for i, j in ((a, b), (b, a)):
            got = _run(gpu, store, F.MAX_MOVES, [i], [j])
            want = ref.grid([i], [j], F.MAX_MOVES)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (k, i, j)
            assert (got[3][0, 0] > 0) == (k > 1)


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


@pytest.mark.parametrize('name,budget', [('b10', 1), ('b10', 4096), ('b32', 4096), ('r32', 16)])
def test_outputs_without_the_restatement(gpu, name, budget):
    from graphembedding_amd.ged import ged_grid
    store, _ = RC.store(name)
    G = len(store)
    ub, lb, mp, mv = _grid(gpu, name, budget)
    ub0, lb0 = (t.cpu().numpy() for t in ged_grid(store, bounds=True, device=gpu))
    assert (lb <= ub).all() and (ub <= ub0).all() and (ub < ub0).any()
    assert np.array_equal(lb, lb0)                           # the descent proves nothing itself
    assert ((ub < ub0) <= (mv > 0)).all() and not mv[lb0 == ub0].any()
    gs = [_plain(store, g) for g in range(G)]
    for a in range(G):
        for b in range(G):
            n1 = len(gs[a][0])
            assert (mp[a, b, n1:] == -1).all()
            assert _induced(gs[a], gs[b], [int(x) for x in mp[a, b, :n1]]) == ub[a, b], (a, b)
    d = np.arange(G)
    assert not ub[d, d].any() and not lb[d, d].any() and not mv[d, d].any()
    if name == 'b10' and budget == 4096:                     # the figures of the full set
        assert int((ub < ub0).sum()) == 71 and int((ub - lb).sum()) == 208
        assert int((ub0 - lb0).sum()) == 536 and int((ub == lb).sum()) == 101


@pytest.mark.parametrize('shape,ld', [((3, 5), 8), ((7, 9), 12), ((13, 11), 11)],
                         ids=['3x5', '7x9', '13x11'])
def test_grid_shapes_indices_and_ld(gpu, shape, ld):
    """Permuted and repeated ids and ld > n, in grids whose m * n is no multiple of the
    workgroup's pairs; the same pair at several grid positions and in launches of several sizes
    gives the same result, and two runs are bitwise equal."""
    store, ref = RC.store('b10')
    G = len(store)
    rng = np.random.default_rng(sum(shape))
    q, db = rng.integers(0, G, size=shape[0]), rng.permutation(np.arange(shape[1]) % G)
    assert (shape[0] * shape[1]) % 4
    for budget in (1, 1024):
        got = _run(gpu, store, budget, q, db, ld=ld)
        want = ref.grid(q, db, budget)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        again = _run(gpu, store, budget, q, db, ld=ld)
        assert all(np.array_equal(g, a) for g, a in zip(got, again))
        full = _grid(gpu, 'b10', budget)
        for g, f in zip(got, full):
            assert np.array_equal(g, f[np.ix_(q, db)])


def test_one_pair_alone_and_inside_a_grid(gpu):
    for name in ('b10', 'b32'):
        store, _ = RC.store(name)
        full = _grid(gpu, name, F.MAX_MOVES)
        assert full[0].size % 4                                # whole grids: odd pair counts
        a, b = np.unravel_index(int(np.argmax(full[3])), full[3].shape)   # the most moves
        for i, j in ((a, b), (b, a), (0, 5), (3, 4), (9, 10)):
            one = _run(gpu, store, F.MAX_MOVES, [i], [j], ld=3)
            for o, f in zip(one, full):
                assert o.shape[:2] == (1, 1) and np.array_equal(o[0, 0], f[i, j]), (name, i, j)


def test_unservable_entries_read_minus_one_and_leave_the_rest(gpu):
    import copy

    from graphembedding_amd import _lib
    from graphembedding_amd.ged import ged_grid
    store, _ = RC.store('b10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    budget = 7
    full = _grid(gpu, 'b10', budget)
    q = np.array([3, -1, 7, 4, G, 5])
    db = np.array([9, 4, 3, 2 ** 31 - 1, 7, 2])
    ub, lb, mp, mv, status = _run(gpu, holed, budget, q, db, return_status=True)
    assert int(status[0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    bad_q, bad_db = [1, 3, 4], [1, 3]
    for out in (ub, lb, mv):
        assert (out[bad_q] == -1).all() and (out[:, bad_db] == -1).all()
    assert (mp[bad_q] == -1).all() and (mp[:, bad_db] == -1).all()
    gq, gdb = [0, 2, 5], [0, 2, 4, 5]
    for out, f in zip((ub, lb, mp, mv), full):
        assert np.array_equal(out[np.ix_(gq, gdb)], f[np.ix_(q[gq], db[gdb])])
    assert (mv[np.ix_(gq, gdb)] > 0).any()
    assert int(_run(gpu, holed, 7, [0, G], [1], return_status=True)[4][0]) == _lib.SG_ERR_ARG
    assert int(_run(gpu, holed, 7, [0, 4], [1], return_status=True)[4][0]) == _lib.SG_ERR_SHAPE
    assert int(_run(gpu, holed, 7, [0, 3], [1], return_status=True)[4][0]) == 0
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_refine_grid: SG_ERR_SHAPE'):
        ged_grid(holed, [4], [1], device=gpu, refine_moves=7)
    grown = copy.copy(store)                                  # a node count above n_max
    grown.n = store.n.copy()
    grown.n[4] = store.n_max + 1
    grown._dev = None
    out = _run(gpu, grown, 7, [3, 4], [4, 9], return_status=True)
    assert int(out[4][0]) == _lib.SG_ERR_SHAPE
    assert (out[0] == [[-1, full[0][3, 9]], [-1, -1]]).all()
    assert (out[3] == [[-1, full[3][3, 9]], [-1, -1]]).all()


def test_map_out_and_moves_out_may_be_null(gpu):
    from graphembedding_amd.ged import ged_grid
    store, _ = RC.store('b10')
    full = _grid(gpu, 'b10', 4096)
    ub, lb = (t.cpu().numpy() for t in ged_grid(store, bounds=True, refine_moves=4096,
                                                device=gpu))
    assert np.array_equal(ub, full[0]) and np.array_equal(lb, full[1])
    ub, lb, mv = (t.cpu().numpy() for t in ged_grid(store, bounds=True, moves=True,
                                                    refine_moves=4096, device=gpu))
    assert np.array_equal(ub, full[0]) and np.array_equal(mv, full[3])
    ub, mp = (t.cpu().numpy() for t in ged_grid(store, mapping=True, refine_moves=4096,
                                                device=gpu))
    assert np.array_equal(ub, full[0]) and np.array_equal(mp, full[2])
    only = ged_grid(store, refine_moves=4096, device=gpu).cpu().numpy()     # ub alone
    assert np.array_equal(only, full[0])


BIG = {'b10': (513, 387, 391), 'b32': (67, 45, 45)}


@pytest.mark.parametrize('name', sorted(BIG))
def test_a_grid_of_many_repeated_ids(gpu, name):
    """Several hundred by several hundred pairs of b10 (and a smaller grid of b32) under seeded
    draws of ids, m * n no multiple of the workgroup's pairs, ld > n on b10: every output equals
    the cached reference indexed by the ids, and the columns n .. ld-1 keep what they held."""
    import torch

    from graphembedding_amd import _lib
    store, ref = RC.store(name)
    G = len(store)
    m, n, ld = BIG[name]
    nm = store.n_max
    assert (m * n) % 4
    rng = np.random.default_rng(m + n)
    q = rng.permutation(np.concatenate([np.arange(G), rng.integers(0, G, size=m - G)]))
    db = rng.permutation(np.concatenate([np.arange(G), rng.integers(0, G, size=n - G)]))
    want = ref.grid(np.arange(G), np.arange(G), F.MAX_MOVES)
    dev_store = store.to_device(gpu)
    dev = dev_store[0].device
    qd = torch.as_tensor(q, dtype=torch.int32, device=dev)
    dbd = torch.as_tensor(db, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.ged_refine_grid_workspace_bytes(m, n, nm) // 4 + 1, dtype=torch.int32,
                     device=dev)
    ub = torch.full((m, ld), -7, dtype=torch.int32, device=dev)
    lb = torch.full((m, ld), -8, dtype=torch.int32, device=dev)
    mv = torch.full((m, ld), -9, dtype=torch.int32, device=dev)
    mp = torch.full((m, n, nm), -5, dtype=torch.int8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.ged_refine_grid(dev_store, nm, qd, m, dbd, n, F.MAX_MOVES, ub, ld, lb, mp, mv, status, ws)
    assert int(status.item()) == 0
    ub, lb, mv, mp = ub.cpu().numpy(), lb.cpu().numpy(), mv.cpu().numpy(), mp.cpu().numpy()
    for out, sentinel in ((ub, -7), (lb, -8), (mv, -9)):
        assert (out[:, n:] == sentinel).all()
    ix = np.ix_(q, db)
    assert np.array_equal(ub[:, :n], want[0][ix])
    assert np.array_equal(lb[:, :n], want[1][ix])
    assert np.array_equal(mp, want[2][ix])
    assert np.array_equal(mv[:, :n], want[3][ix])
    assert (mv[:, :n] > 0).any()


# ---- the Python layer ---------------------------------------------------------------------
def test_ged_matrix_pair_and_distance_ged(gpu):
    from graphembedding_amd import distance, ged
    graphs = RC.graphs('b10')
    store, _ = RC.store('b10')
    ubk, lbk, _, _ = _grid(gpu, 'b10', 1024)
    dm, proven = ged.ged_matrix(graphs[:6], device=gpu, refine_moves=1024)
    sub = ged.store_of_graphs(graphs[:6])
    wub, wlb = (t.cpu().numpy() for t in ged.ged_grid(sub, bounds=True, refine_moves=1024,
                                                      device=gpu))
    assert dm.dtype == np.int64 and proven.dtype == bool
    assert np.array_equal(dm, wub) and np.array_equal(proven, wub == wlb)
    dmk, provenk = ged.ged_matrix(store, device=gpu, refine_moves=1024)
    assert np.array_equal(dmk, ubk) and np.array_equal(provenk, ubk == lbk)
    assert not provenk.all()
    u, l = ged.ged_pair(graphs[2], graphs[5], device=gpu, refine_moves=1024)
    assert u == distance.ged(graphs[2], graphs[5], 'bpswap')
    u0, l0 = ged.ged_pair(graphs[2], graphs[5], device=gpu)
    assert l == l0 <= u <= u0
    assert (u, l) == F.refine_pair(*_nx_pair(ged, graphs[2], graphs[5]), 1024)[:2]
    assert distance.ged(graphs[0], graphs[0], 'bpswap') == 0
    with pytest.raises(ValueError, match='mutually exclusive'):
        ged.ged_grid(store, exact_budget=7, refine_moves=7, device=gpu)
    with pytest.raises(ValueError, match='mutually exclusive'):
        ged.ged_grid(store, beam_width=7, refine_moves=7, device=gpu)
    with pytest.raises(ValueError, match='refine_moves'):
        ged.ged_grid(store, moves=True, device=gpu)
    with pytest.raises(ValueError, match='both assignment orders'):
        ged.ged_grid(store, refine_moves=7, both_orders=False, device=gpu)
    with pytest.raises(_lib_error(), match='SG_ERR_UNSUPPORTED'):
        ged.ged_grid(store, refine_moves=4097, device=gpu)
    csr = ged.csr_store_of_graphs(graphs[:6])
    with pytest.raises(ValueError, match='no refine_moves'):
        ged.ged_grid(csr, refine_moves=7, device=gpu)
    with pytest.raises(ValueError, match='no refine_moves'):
        ged.ged_grid(csr, moves=True, device=gpu)


def _lib_error():
    from graphembedding_amd import _lib
    return _lib.SiameseHipError


def _nx_pair(ged, g1, g2):
    """The restatement's graphs of two networkx graphs, through the two-graph store ged_pair
    builds."""
    import _ged_restatement as R
    s = ged.store_of_graphs([g1, g2])
    return R.graph_of_store(s, 0), R.graph_of_store(s, 1)


def test_refine_label_matrix_logs_and_has_a_zero_diagonal(gpu, caplog):
    import logging

    from graphembedding_amd import ged
    store, _ = RC.store('b10')
    with caplog.at_level(logging.INFO, logger='graphembedding_amd.ged'):
        dm = ged.refine_label_matrix(store, device=gpu)
    full = _grid(gpu, 'b10', 1024)
    assert '{} of 169 pairs left unproven within 1024 moves per start'.format(
        int((full[0] != full[1]).sum())) in caplog.text
    assert dm.dtype == np.int64 and np.array_equal(dm, full[0])
    assert not np.diag(dm).any()                 # the seed already has lb == ub there
    few = ged.refine_label_matrix(store, moves=1, device=gpu)
    assert (few >= dm).all() and (few > dm).any()


def test_load_graph_set_with_refined_labels(gpu, caplog):
    import logging

    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.ged import ged_grid
    with caplog.at_level(logging.INFO, logger='graphembedding_amd.ged'):
        gs = load_graph_set('syn_aids80nef', ged='bpswap', device=gpu)
    assert 'of 6400 pairs left unproven within 1024 moves per start' in caplog.text
    ub, lb = (t.cpu().numpy() for t in ged_grid(gs.store, bounds=True, device=gpu))
    assert gs.ged.dtype == np.int64 and gs.ged.shape == (80, 80)
    assert (gs.ged <= ub).all() and (gs.ged >= lb).all() and (gs.ged < ub).any()
    assert not np.diag(gs.ged).any()


def test_train_main_with_refined_labels(gpu):
    from graphembedding_amd.config import Flags
    from graphembedding_amd.ged import ged_matrix
    from graphembedding_amd.train import main
    f = Flags(ged_labels='bpswap', iters=3, dataset='syn_aids80nef', n_max=10,
              node_feat_order='sorted', test_path='embed')
    tr, _, (data, dc, _) = main(f, device=gpu, return_objects=True)
    idx, dm = dc.matrix
    by_gid = {g.graph['gid']: g for g in list(data.orig_train_graphs) +
              [data.test_data.gs[i].nxgraph for i in range(data.m)]}
    graphs = [by_gid[k] for k in sorted(idx, key=idx.get)]
    want, _ = ged_matrix(graphs, device=gpu, refine_moves=1024)
    assert dm.shape == (80, 80) and np.array_equal(dm, want)
    losses = np.asarray(tr[0], dtype=np.float64)
    assert losses.size == 3 and np.isfinite(losses).all()
