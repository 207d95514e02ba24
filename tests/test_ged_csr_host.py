"""The numpy specification of the graph-store GED bounds (tests/_ged_csr_restatement.py, read
from CsrStore arrays) without a GPU: on the dense suites' graph sets it equals the dense
restatement bit for bit, and above 32 nodes its optima are scipy's, lb <= ub and the assignment
is injective and induces ub."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _ged_csr_restatement as C
import _ged_restatement as R
from test_gpu_ged import _graphs, _random_graph


@pytest.mark.parametrize('name', ['cap10', 'cap32', 'tie10', 'tie32'])
def test_csr_restatement_equals_the_dense_restatement(name):
    from graphembedding_amd.ged import csr_store_of_graphs, store_of_graphs
    graphs = _graphs(name)
    dense = R.GridReference(store_of_graphs(graphs))
    csr = C.GridReference(csr_store_of_graphs(graphs))
    G = len(graphs)
    for a in range(G):
        for b in range(G):
            ub, lb, phi = csr.pair(a, b)
            wub, wlb, wphi = dense.pair(a, b)
            assert (ub, lb) == (wub, wlb), (a, b)
            assert np.array_equal(phi, wphi), (a, b)


def _big_pair(n1, n2, types):
    rng = np.random.default_rng(1000 * n1 + n2)
    return [_random_graph(rng, n1, 0, types=types, p_extra=0.02),
            _random_graph(rng, n2, 1, types=types, p_extra=0.02)]


FOUR = ('C', 'N', 'O', 'S')


@pytest.mark.parametrize('n1,n2,types', [(33, 31, FOUR), (40, 90, FOUR), (128, 129, FOUR),
                                         (130, 130, ('C',))],
                         ids=['33x31', '40x90', '128x129', '130x130_one_type'])
def test_above_32_nodes_against_scipy(n1, n2, types):
    from graphembedding_amd.ged import csr_store_of_graphs
    store = csr_store_of_graphs(_big_pair(n1, n2, types))
    g1, g2 = C.graph_of_store(store, 0), C.graph_of_store(store, 1)
    opts = {}
    for w in (1, 2):
        M = C.cost_matrix(g1, g2, w)
        p, opts[w] = C.lsap(M)
        r, c = linear_sum_assignment(M)
        assert opts[w] == int(M[r, c].sum()), w
        assert sorted(p.tolist()) == list(range(n1 + n2))
        if w == 1:
            phi = C.phi_of(p, n1, n2)
    kept = phi[phi >= 0]
    assert len(set(kept.tolist())) == kept.size and (kept < n2).all()
    ub = C.induced_cost(g1, g2, phi)
    assert (ub, phi.tolist()) == (C.upper_bound(g1, g2)[0], C.upper_bound(g1, g2)[1].tolist())
    # the edit path of phi, edge by edge
    (t1, A1), (t2, A2) = g1, g2
    cost = int((phi < 0).sum()) + (n2 - kept.size) + sum(
        int(t1[a] != t2[phi[a]]) for a in range(n1) if phi[a] >= 0)
    for a in range(n1):
        for b in range(a):
            if A1[a, b] and not (phi[a] >= 0 and phi[b] >= 0 and A2[phi[a], phi[b]]):
                cost += 1
    inv = {int(f): a for a, f in enumerate(phi) if f >= 0}
    for x in range(n2):
        for y in range(x):
            if A2[x, y] and not (x in inv and y in inv and A1[inv[x], inv[y]]):
                cost += 1
    assert cost == ub
    lb = (opts[2] + 1) // 2
    assert lb == C.lower_bound(g1, g2) and 0 <= lb <= ub
