"""Beam-search GED on the GPU (include/siamese_ged_beam.h) on what test_gpu_ged_beam.py never
launches: the sets of _ged_beam_classes.py (one-type dense graphs at capacity 32, edgeless graphs,
forests, 29 types, planted near-copies, capacities 1, 7, 16, 17, 31 and 32) and a grid of more
than 2^20 pairs.  ub, lb, map_out and expanded_out equal tests/_ged_beam_restatement.py bit for
bit; then checks that use no restatement.  test_ged_beam_classes_host.py shows on the host which
pairs of these grids are truncated or searched to the end and that the dense set takes the state
word, the selection and the masks to their limits."""
import numpy as np
import pytest

import _ged_beam_cases as BC
import _ged_beam_classes as BK
import _ged_classes as K

pytestmark = pytest.mark.gpu

CASES = [(name, w) for name, widths in BK.GRIDS for w in widths]
_OUT = {}


def _run(gpu, store, width, q=None, db=None, **kw):
    from graphembedding_amd.ged import ged_grid
    out = ged_grid(store, q, db, bounds=True, mapping=True, expanded=True, beam_width=width,
                   device=gpu, **kw)
    return [t.cpu().numpy() for t in out]


def _grid(gpu, name, width):
    """(ub, lb, map, expanded) of a whole set, one call per (set, width)."""
    if (name, width) not in _OUT:
        _OUT[(name, width)] = _run(gpu, BK.store(name)[0], width)
    return _OUT[(name, width)]


def _b10(gpu, width):
    if ('b10', width) not in _OUT:
        _OUT[('b10', width)] = _run(gpu, BC.store('b10')[0], width)
    return _OUT[('b10', width)]


# ---- 1. against the restatement -------------------------------------------------------------
@pytest.mark.parametrize('name,width', CASES, ids=['{}-w{}'.format(*c) for c in CASES])
def test_grids_equal_the_restatement(gpu, name, width):
    store, ref = BK.store(name)
    G = len(store)
    ub, lb, mp, ex = _grid(gpu, name, width)
    wub, wlb, wmp, wex = ref.grid(range(G), range(G), width)
    assert ub.dtype == np.int32 and lb.dtype == np.int32 and mp.dtype == np.int8
    assert ex.dtype == np.int32 and mp.shape == (G, G, BK.capacity(name))
    assert np.array_equal(ex, wex), np.argwhere(ex != wex)[:5]
    assert np.array_equal(ub, wub), np.argwhere(ub != wub)[:5]
    assert np.array_equal(lb, wlb), np.argwhere(lb != wlb)[:5]
    assert np.array_equal(mp, wmp), np.argwhere(mp != wmp)[:5]
    assert (ex >= 0).all() and (ex <= 1 + (store.n[:, None] - 1) * width).all()
    assert (ex > 0).any() == (name not in BK.NEVER_SEARCHED)


# ---- 2. without the restatement -------------------------------------------------------------
def _induced(g1, g2, phi):
    """The cost of the edit path of phi between two networkx graphs."""
    n1, n2 = g1.number_of_nodes(), g2.number_of_nodes()
    kept = [x for x in phi if x >= 0]
    assert len(phi) == n1 and len(set(kept)) == len(kept) and all(x < n2 for x in kept)
    subs = sum(1 for a, x in enumerate(phi) if x >= 0 and
               g1.nodes[a]['type'] != g2.nodes[x]['type'])
    both = sum(1 for a, b in g1.edges() if phi[a] >= 0 and phi[b] >= 0 and
               g2.has_edge(phi[a], phi[b]))
    return ((n1 - len(kept)) + (n2 - len(kept)) + subs + g1.number_of_edges() +
            g2.number_of_edges() - 2 * both)


@pytest.mark.parametrize('name,width', CASES, ids=['{}-w{}'.format(*c) for c in CASES])
def test_the_map_induces_ub(gpu, name, width):
    gs = BK.graphs(name)
    ub, lb, mp, ex = _grid(gpu, name, width)
    assert (lb <= ub).all() and (lb >= 0).all()
    for a, g1 in enumerate(gs):
        for b, g2 in enumerate(gs):
            n1 = g1.number_of_nodes()
            assert (mp[a, b, n1:] == -1).all()
            assert _induced(g1, g2, [int(x) for x in mp[a, b, :n1]]) == ub[a, b], (a, b)
    d = np.arange(len(gs))
    assert not ub[d, d].any() and not lb[d, d].any() and not ex[d, d].any()


@pytest.mark.parametrize('name', ['dense32', 'edge0'])
def test_closed_forms(gpu, name):
    known = BK.closed_form(name)
    n_proven = n_open = 0
    for width in dict(BK.GRIDS)[name]:
        ub, lb, _, _ = _grid(gpu, name, width)
        for (a, b), value in known.items():
            assert lb[a, b] <= value <= ub[a, b], (width, a, b)
            assert lb[a, b] != ub[a, b] or ub[a, b] == value, (width, a, b)
            n_proven += lb[a, b] == ub[a, b]
            n_open += lb[a, b] != ub[a, b]
    assert n_proven > 0 and (n_open > 0 or name == 'edge0')


@pytest.mark.parametrize('name', ['planted16', 'planted9'])
def test_planted_copies_are_found(gpu, name):
    gs = BK.graphs(name)
    ub, lb, mp, _ = _grid(gpu, name, 128)
    for a, b in ((0, 1), (1, 0)):
        assert ub[a, b] == 0 and lb[a, b] == 0
        assert K.is_isomorphism(gs[a], gs[b], [int(x) for x in mp[a, b]])
    assert K.permutation(name) != sorted(K.permutation(name))      # no identity
    for (a, b), rule in K.known(name).items():
        assert lb[a, b] <= rule[1]
        assert rule[0] == 'le' or lb[a, b] != ub[a, b] or ub[a, b] == rule[1]


# ---- 3. capacity independence ---------------------------------------------------------------
@pytest.mark.parametrize('c', BK.RESTORED)
def test_results_do_not_depend_on_the_store_capacity(gpu, c):
    store = BK.restored(c)
    G = len(store)
    for width in BK.RESTORED_WIDTHS:
        ub, lb, mp, ex = _run(gpu, store, width)
        wub, wlb, wmp, wex = _b10(gpu, width)
        assert mp.shape == (G, G, c) and wmp.shape == (G, G, 10)
        assert np.array_equal(ub, wub) and np.array_equal(lb, wlb) and np.array_equal(ex, wex)
        assert np.array_equal(mp[..., :10], wmp) and (mp[..., 10:] == -1).all()
        assert (ex > 0).any() and (ub != lb).any()


# ---- 4. a grid of more than 2^20 pairs ------------------------------------------------------
def test_a_grid_of_more_than_2_20_pairs(gpu):
    """1025 x 1024 pairs at width 1 with ld = 1031: the launch has two grid rows and the second
    holds the 1024 pairs of query row 1024.  Every output equals the whole-set result indexed
    by the ids, and the columns n .. ld-1 of ub, lb and expanded keep what they held.
    Measured on an MI355X: 0.06 s for the call, 0.1 s for the test."""
    import torch

    from graphembedding_amd import _lib
    store, _ = BC.store('b10')
    q, db = BK.big_ids()
    m, n, ld, nm = BK.BIG_M, BK.BIG_N, BK.BIG_LD, store.n_max
    assert BK.grid_rows(m, n)[1] == 2
    full = _b10(gpu, BK.BIG_WIDTH)
    dev_store = store.to_device(gpu)
    dev = dev_store[0].device
    qd = torch.as_tensor(q, dtype=torch.int32, device=dev)
    dbd = torch.as_tensor(db, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.ged_beam_grid_workspace_bytes(m, n, nm) // 4 + 1, dtype=torch.int32,
                     device=dev)
    ub = torch.full((m, ld), -7, dtype=torch.int32, device=dev)
    lb = torch.full((m, ld), -8, dtype=torch.int32, device=dev)
    ex = torch.full((m, ld), -9, dtype=torch.int32, device=dev)
    mp = torch.full((m, n, nm), -5, dtype=torch.int8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    import time
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    _lib.ged_beam_grid(dev_store, nm, qd, m, dbd, n, BK.BIG_WIDTH, ub, ld, lb, mp, ex, status, ws)
    torch.cuda.synchronize(dev)
    print('the 1025 x 1024 call took', time.perf_counter() - t0, 's on the device')
    assert int(status.item()) == 0
    ub, lb, ex, mp = ub.cpu().numpy(), lb.cpu().numpy(), ex.cpu().numpy(), mp.cpu().numpy()
    for out, sentinel in ((ub, -7), (lb, -8), (ex, -9)):
        assert (out[:, n:] == sentinel).all()
    ix = np.ix_(q, db)
    assert np.array_equal(ub[:, :n], full[0][ix])
    assert np.array_equal(lb[:, :n], full[1][ix])
    assert np.array_equal(mp, full[2][ix])
    assert np.array_equal(ex[:, :n], full[3][ix])
    assert (ex[1024, :n] > 0).any() and len(np.unique(ub[1024, :n])) > 1   # the second grid row


# ---- 5. determinism -------------------------------------------------------------------------
def test_two_runs_of_the_dense_grid_are_bitwise_equal(gpu):
    first = _grid(gpu, 'dense32', 128)
    again = _run(gpu, BK.store('dense32')[0], 128)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert (first[3] > 1 + 30 * 128).any()
