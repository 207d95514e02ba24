"""Beam-search GED on the GPU (include/siamese_ged_beam.h): ub, lb, map_out and expanded_out of
sg_ged_beam_grid equal tests/_ged_beam_restatement.py bit for bit at both store capacities and
at the widths around the wavefront's 64 lanes (test_ged_beam_host.py shows which pairs of these
grids are truncated, run to the end, pruned empty or seeded by the 2->1 order).  Then checks
that use no restatement (the induced cost of map_out, the bipartite call's bounds, the exact
call's distances), grid layout and position independence, entries the call cannot serve, and
the Python layer."""
import numpy as np
import pytest

import _ged_beam_cases as BC
import _ged_exact_cases as C

pytestmark = pytest.mark.gpu

CASES = [(name, w, q, db) for name, widths, q, db in BC.GRIDS for w in widths]
_OUT = {}


def _run(gpu, store, width, q=None, db=None, **kw):
    from graphembedding_amd.ged import ged_grid
    out = ged_grid(store, q, db, bounds=True, mapping=True, expanded=True, beam_width=width,
                   device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


def _grid(gpu, name, width, q=None, db=None):
    """(ub, lb, map, expanded) of a grid of a set, one call per (set, width, grid)."""
    key = (name, width, q, db)
    if key not in _OUT:
        _OUT[key] = _run(gpu, BC.store(name)[0], width, q, db)
    return _OUT[key]


@pytest.mark.parametrize('name,width,q,db', CASES,
                         ids=['{}-w{}{}'.format(c[0], c[1], '' if c[2] is None else '-large')
                              for c in CASES])
def test_grids_equal_the_restatement(gpu, name, width, q, db):
    store, ref = BC.store(name)
    ub, lb, mp, ex = _grid(gpu, name, width, q, db)
    qi, dbi = BC.ids(name, q), BC.ids(name, db)
    wub, wlb, wmp, wex = ref.grid(qi, dbi, width)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert ex.dtype == np.int32 and mp.shape == (len(qi), len(dbi), store.n_max)
    assert np.array_equal(ex, wex), np.argwhere(ex != wex)[:5]
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    n1 = store.n[qi][:, None]
    assert (ex >= 0).all() and (ex <= 1 + (n1 - 1) * width).all()
    if width == 0:
        assert not ex.any()
    else:
        assert (ex > 0).any() and (ub != lb).any()


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


@pytest.mark.parametrize('name,width', [('b10', 1), ('b10', 65), ('b10', 128), ('b32', 7)])
def test_outputs_without_the_restatement(gpu, name, width):
    from graphembedding_amd.ged import ged_grid
    store, _ = BC.store(name)
    G = len(store)
    ub, lb, mp, ex = _grid(gpu, name, width)
    ub0, lb0 = (t.cpu().numpy() for t in ged_grid(store, bounds=True, device=gpu))
    assert (lb <= ub).all() and (ub <= ub0).all() and ((ub < ub0).any() or width == 1)
    assert ((lb == ub) | (lb == lb0)).all()                  # lb is ub, or the bipartite lb
    gs = [_plain(store, g) for g in range(G)]
    for a in range(G):
        for b in range(G):
            n1 = len(gs[a][0])
            assert (mp[a, b, n1:] == -1).all()
            assert _induced(gs[a], gs[b], [int(x) for x in mp[a, b, :n1]]) == ub[a, b], (a, b)
    d = np.arange(G)
    assert not ub[d, d].any() and not lb[d, d].any() and not ex[d, d].any()
    # pairs of at most 10 nodes that both calls prove: the same distance
    xub, xlb = (t.cpu().numpy() for t in ged_grid(store, bounds=True, device=gpu,
                                                  exact_budget=C.PROVE_BUDGET))
    small = np.maximum(store.n[:, None], store.n[None, :]) <= 10
    both = small & (ub == lb) & (xub == xlb)
    assert np.array_equal(ub[both], xub[both]) and both.any()
    assert (both & (ex > 0)).any() or name == 'b32'      # b32's small graphs meet at the seed
    assert (ub[small & (xub == xlb)] >= xub[small & (xub == xlb)]).all()


@pytest.mark.parametrize('shape,ld', [((3, 5), 8), ((7, 9), 12), ((13, 11), 11)],
                         ids=['3x5', '7x9', '13x11'])
def test_grid_shapes_indices_and_ld(gpu, shape, ld):
    """Permuted and repeated ids and ld > n; the same pair at several grid positions and in
    launches of several sizes gives the same result, and two runs are bitwise equal."""
    store, ref = BC.store('b10')
    G = len(store)
    rng = np.random.default_rng(sum(shape))
    q, db = rng.integers(0, G, size=shape[0]), rng.permutation(np.arange(shape[1]) % G)
    for width in (2, 80):
        got = _run(gpu, store, width, q, db, ld=ld)
        want = ref.grid(q, db, width)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        again = _run(gpu, store, width, q, db, ld=ld)
        assert all(np.array_equal(g, a) for g, a in zip(got, again))
        full = _grid(gpu, 'b10', width)
        for g, f in zip(got, full):
            assert np.array_equal(g, f[np.ix_(q, db)])


def test_one_pair_alone_and_inside_a_grid(gpu):
    store, _ = BC.store('b10')
    for width in (7, 128):
        full = _grid(gpu, 'b10', width)
        a, b = np.unravel_index(int(np.argmax(full[3])), full[3].shape)   # the costliest pair
        for i, j in ((a, b), (0, 9), (3, 4), (11, 12)):
            one = _run(gpu, store, width, [i], [j], ld=3)
            for o, f in zip(one, full):
                assert o.shape[:2] == (1, 1) and np.array_equal(o[0, 0], f[i, j]), (i, j)


def test_unservable_entries_read_minus_one_and_leave_the_rest(gpu):
    import copy

    from graphembedding_amd import _lib
    from graphembedding_amd.ged import ged_grid
    store, _ = BC.store('b10')
    G = len(store)
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    holed._dev = None
    width = 7
    full = _grid(gpu, 'b10', width)
    q = np.array([3, -1, 7, 4, G, 5])
    db = np.array([9, 4, 3, 2 ** 31 - 1, 7, 2])
    ub, lb, mp, ex, status = _run(gpu, holed, width, q, db, return_status=True)
    assert int(status[0]) in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    bad_q, bad_db = [1, 3, 4], [1, 3]
    for out in (ub, lb, ex):
        assert (out[bad_q] == -1).all() and (out[:, bad_db] == -1).all()
    assert (mp[bad_q] == -1).all() and (mp[:, bad_db] == -1).all()
    gq, gdb = [0, 2, 5], [0, 2, 4, 5]
    for out, f in zip((ub, lb, mp, ex), full):
        assert np.array_equal(out[np.ix_(gq, gdb)], f[np.ix_(q[gq], db[gdb])])
    assert (ex[np.ix_(gq, gdb)] > 0).any()
    assert int(_run(gpu, holed, 7, [0, G], [1], return_status=True)[4][0]) == _lib.SG_ERR_ARG
    assert int(_run(gpu, holed, 7, [0, 4], [1], return_status=True)[4][0]) == _lib.SG_ERR_SHAPE
    assert int(_run(gpu, holed, 7, [0, 3], [1], return_status=True)[4][0]) == 0
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_beam_grid: SG_ERR_SHAPE'):
        ged_grid(holed, [4], [1], device=gpu, beam_width=7)


def test_map_out_and_expanded_out_may_be_null(gpu):
    from graphembedding_amd.ged import ged_grid
    store, _ = BC.store('b10')
    full = _grid(gpu, 'b10', 7)
    ub, lb = (t.cpu().numpy() for t in ged_grid(store, bounds=True, beam_width=7, device=gpu))
    assert np.array_equal(ub, full[0]) and np.array_equal(lb, full[1])
    ub, lb, ex = (t.cpu().numpy() for t in ged_grid(store, bounds=True, expanded=True,
                                                    beam_width=7, device=gpu))
    assert np.array_equal(ub, full[0]) and np.array_equal(ex, full[3])
    only = ged_grid(store, beam_width=7, device=gpu).cpu().numpy()     # ub alone
    assert np.array_equal(only, full[0])


# ---- the Python layer ---------------------------------------------------------------------
def test_ged_matrix_pair_and_distance_ged(gpu):
    from graphembedding_amd import distance, ged
    graphs = BC.graphs('b10')
    store, _ = BC.store('b10')
    ub7, lb7, _, _ = _grid(gpu, 'b10', 7)
    dm, proven = ged.ged_matrix(graphs[:6], device=gpu, beam_width=7)
    sub = ged.store_of_graphs(graphs[:6])
    wub, wlb = (t.cpu().numpy() for t in ged.ged_grid(sub, bounds=True, beam_width=7, device=gpu))
    assert dm.dtype == np.int64 and proven.dtype == bool
    assert np.array_equal(dm, wub) and np.array_equal(proven, wub == wlb)
    dm7, proven7 = ged.ged_matrix(store, device=gpu, beam_width=7)
    assert np.array_equal(dm7, ub7) and np.array_equal(proven7, ub7 == lb7) and not proven7.all()
    u, l = ged.ged_pair(graphs[2], graphs[5], device=gpu, beam_width=7)
    assert u == distance.ged(graphs[2], graphs[5], 'lbeam7')
    assert l <= u <= ged.ged_pair(graphs[2], graphs[5], device=gpu)[0]
    assert distance.ged(graphs[0], graphs[0], 'lbeam80') == 0
    with pytest.raises(ValueError, match='mutually exclusive'):
        ged.ged_grid(store, exact_budget=7, beam_width=7, device=gpu)
    with pytest.raises(ValueError, match='beam_width'):
        ged.ged_grid(store, expanded=True, device=gpu)
    with pytest.raises(ValueError, match='both assignment orders'):
        ged.ged_grid(store, beam_width=7, both_orders=False, device=gpu)


def test_load_graph_set_with_beam_labels(gpu, caplog):
    import logging

    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.ged import ged_grid
    with caplog.at_level(logging.INFO, logger='graphembedding_amd.ged'):
        gs = load_graph_set('syn_aids80nef', ged='lbeam7', device=gpu)
    assert 'of 6400 pairs left unproven at width 7' in caplog.text
    ub, lb = (t.cpu().numpy() for t in ged_grid(gs.store, bounds=True, device=gpu))
    assert gs.ged.dtype == np.int64 and gs.ged.shape == (80, 80)
    assert (gs.ged <= ub).all() and (gs.ged >= lb).all() and (gs.ged < ub).any()
    assert not np.diag(gs.ged).any()


def test_train_main_with_beam_labels(gpu):
    from graphembedding_amd.config import Flags
    from graphembedding_amd.ged import ged_matrix
    from graphembedding_amd.train import main
    f = Flags(ged_labels='lbeam7', iters=3, dataset='syn_aids80nef', n_max=10,
              node_feat_order='sorted', test_path='embed')
    tr, _, (data, dc, _) = main(f, device=gpu, return_objects=True)
    idx, dm = dc.matrix
    by_gid = {g.graph['gid']: g for g in list(data.orig_train_graphs) +
              [data.test_data.gs[i].nxgraph for i in range(data.m)]}
    graphs = [by_gid[k] for k in sorted(idx, key=idx.get)]
    want, _ = ged_matrix(graphs, device=gpu, beam_width=7)
    assert dm.shape == (80, 80) and np.array_equal(dm, want)
    losses = np.asarray(tr[0], dtype=np.float64)
    assert losses.size == 3 and np.isfinite(losses).all()
    with pytest.raises(RuntimeError, match='Unknown ged_labels'):
        main(Flags(ged_labels='beam80', iters=1, dataset='syn_aids80nef', n_max=10), device=gpu)
