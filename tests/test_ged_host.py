"""The yardstick of the device GED bounds (tests/_ged_restatement.py) against independent
solvers, on the host: its assignment cost is scipy's LSAP optimum on both matrices, its phi is
a partial injection, and lb <= exact GED (networkx) <= ub on small random connected graphs."""
import networkx as nx
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _ged_restatement as R


def _random_connected(rng, n, n_types=3, p_extra=0.3):
    A = np.zeros((n, n), dtype=bool)
    for v in range(1, n):
        w = int(rng.integers(0, v))
        A[v, w] = A[w, v] = True
    iu, ju = np.triu_indices(n, 1)
    extra = rng.random(iu.shape[0]) < p_extra
    A[iu[extra], ju[extra]] = True
    A[ju[extra], iu[extra]] = True
    return rng.integers(0, n_types, size=n).astype(np.int64), A


def _nx(g):
    t, A = g
    G = nx.Graph()
    for a in range(len(t)):
        G.add_node(a, type=int(t[a]))
    G.add_edges_from((a, b) for a in range(len(t)) for b in range(a) if A[a, b])
    return G


def _exact(g1, g2):
    d = nx.graph_edit_distance(_nx(g1), _nx(g2), node_match=lambda a, b: a['type'] == b['type'])
    assert d == int(d)
    return int(d)


@pytest.fixture(scope='module')
def small_graphs():
    rng = np.random.default_rng(20)
    return [_random_connected(rng, n) for n in (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 5)]


def test_assignment_cost_is_scipys_optimum_on_both_matrices():
    rng = np.random.default_rng(3)
    gs = [_random_connected(rng, int(n), n_types=int(nt))
          for n, nt in zip(rng.integers(1, 13, size=14), rng.integers(1, 4, size=14))]
    for g1 in gs:
        for g2 in gs:
            for w in (1, 2):
                C = R.cost_matrix(g1, g2, w)
                p, cost = R.lsap(C)
                r, c = linear_sum_assignment(C)
                assert cost == int(C[r, c].sum()), (w, len(g1[0]), len(g2[0]))
                assert sorted(p.tolist()) == list(range(C.shape[0]))     # a permutation
                assert cost == int(C[p, np.arange(C.shape[0])].sum())    # dual sum == primal
                assert cost < R.BIG


def test_lsap_tie_rules_on_a_constant_matrix():
    """Every entry equal: every round's argmin is the smallest unused column, so row i ends on
    column i."""
    p, cost = R.lsap(np.full((6, 6), 3))
    assert p.tolist() == list(range(6)) and cost == 18


def test_phi_is_a_partial_injection(small_graphs):
    for g1 in small_graphs:
        for g2 in small_graphs:
            ub, phi = R.upper_bound(g1, g2)
            kept = [int(x) for x in phi if x >= 0]
            assert len(phi) == len(g1[0])
            assert all(0 <= x < len(g2[0]) for x in kept)
            assert len(set(kept)) == len(kept)
            assert ub == R.induced_cost(g1, g2, phi)


def test_bounds_enclose_the_exact_distance(small_graphs):
    n_exact = 0
    for i, g1 in enumerate(small_graphs):
        for j, g2 in enumerate(small_graphs):
            ub, lb, _ = R.bp_pair(g1, g2, both_orders=False)
            ub2, lb2, _ = R.bp_pair(g1, g2, both_orders=True)
            d = _exact(g1, g2)
            assert lb <= d <= ub2 <= ub, (i, j, lb, d, ub2, ub)
            assert lb2 == lb == R.lower_bound(g2, g1)      # the swapped matrix is the transpose
            # at least |n1 - n2| nodes are inserted or deleted, at 2 each in the doubled matrix
            assert lb >= abs(len(g1[0]) - len(g2[0]))
            n_exact += lb == ub2
            if i == j:
                assert ub == lb == 0
    print('lb == ub on {} of {} pairs'.format(n_exact, len(small_graphs) ** 2))


def test_store_graphs_drop_the_diagonal_and_the_padding():
    from graphembedding_amd.packer import GraphStore

    class MG(object):
        def __init__(self, A, t):
            self.adj, self.types, self.nxgraph = A, np.asarray(t, np.int32), nx.Graph(gid=0)

        def num_nodes(self):
            return len(self.types)

    A = np.array([[.5, .3, 0.], [.3, .5, .2], [0., .2, .5]])
    store = GraphStore([MG(A, [4, 4, 7])], n_max=5)
    t, B = R.graph_of_store(store, 0)
    assert t.tolist() == [4, 4, 7]
    assert B.astype(int).tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
