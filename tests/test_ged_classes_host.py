"""The two GED restatements on the graph classes of tests/_ged_classes.py, on the host, against
oracles that are neither of them: scipy's LSAP optimum, the closed forms and planted bounds of
that module, networkx on the small pairs, and the admissibility check of test_ged_exact_host.py.
Then the budget test_gpu_ged_classes.py proves every pair with, re-derived, and the pairs its
reach assertions need.  The unlimited searches are cached under pytest's cache dir."""
import networkx as nx
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _ged_classes as K
import _ged_exact_restatement as X
import _ged_restatement as R
from test_ged_exact_host import test_h_is_admissible_along_optimal_paths as _admissible


@pytest.fixture(scope='module')
def cache(request, tmp_path_factory):
    if hasattr(request.config, 'cache') and request.config.cache is not None:
        return request.config.cache.mkdir('ged_classes')
    return tmp_path_factory.mktemp('ged_classes')


def _nx_ged(g1, g2):
    d = nx.graph_edit_distance(g1, g2, node_match=lambda a, b: a['type'] == b['type'])
    assert d == int(d)
    return int(d)


@pytest.mark.parametrize('name', K.SETS)
def test_bipartite_restatement_on_every_set(name):
    """Both assignment costs are scipy's optimum, phi is a partial injection that induces ub,
    and lb <= the known distance <= ub."""
    _, ref, _ = K.store(name)
    known = K.known(name)
    G = len(K.graphs(name))
    for a in range(G):
        for b in range(G):
            g1, g2 = ref.graph(a), ref.graph(b)
            opt = {}
            for w in (1, 2):
                C = R.cost_matrix(g1, g2, w)
                p, cost = R.lsap(C)
                r, c = linear_sum_assignment(C)
                assert cost == int(C[r, c].sum()) < R.BIG, (a, b, w)
                assert sorted(p.tolist()) == list(range(C.shape[0]))
                opt[w] = cost
            ub, lb, phi = ref.pair(a, b)
            assert lb == (opt[2] + 1) // 2
            kept = [int(x) for x in phi if x >= 0]
            assert len(phi) == len(g1[0]) and len(set(kept)) == len(kept)
            assert all(0 <= x < len(g2[0]) for x in kept)
            assert R.induced_cost(g1, g2, phi) == ub
            ub = min(ub, ref.pair(b, a)[0])
            assert lb <= ub
            if (a, b) in known:
                kind, v = known[(a, b)]
                assert lb <= v, (a, b, lb, v)
                assert kind == 'le' or v <= ub, (a, b, v, ub)
    if name == 'edge0':                          # no edges: the assignment is the edit path
        assert all(ref.pair(a, b)[0] == ref.pair(a, b)[1] for a in range(G) for b in range(G))


@pytest.mark.parametrize('name', K.SETS)
def test_exact_restatement_with_an_unlimited_budget(name, cache):
    gs = K.graphs(name)
    _, _, ref = K.store(name)
    solved = K.solved(name, cache)
    known = K.known(name)
    assert set(solved) == set(K.searched_pairs(name))
    n_nx = 0
    for (a, b), (ub, lb, phi, e) in solved.items():
        g1, g2 = ref.graph(a), ref.graph(b)
        assert ub == lb and R.induced_cost(g1, g2, phi) == ub, (a, b)      # proven, by a real path
        assert ub == solved[(b, a)][0], (a, b)
        if (a, b) in known:
            assert K.holds(known[(a, b)], ub), (a, b, ub, known[(a, b)])
            if known[(a, b)] == ('eq', 0):
                assert K.is_isomorphism(gs[a], gs[b], phi), (a, b)
        if max(len(g1[0]), len(g2[0])) <= 6:
            assert ub == _nx_ged(gs[a], gs[b]), (a, b)
            n_nx += 1
    assert n_nx >= {'edge0': 9, 'forest': 4, 'types29': 4}.get(name, 1 if name in K.DENSE else 0)
    if name in K.DENSE or name == 'edge0':       # every pair of these has a closed form ...
        missing = [p for p in solved if p not in known]
        assert all(K.DENSE[name][p[0]][1] and K.DENSE[name][p[1]][1] for p in missing)
    if name in K.PLANTED:
        perm = K.permutation(name)
        assert K.is_isomorphism(gs[0], gs[1], perm) and perm != sorted(perm)
        assert solved[(0, 1)][0] == 0 and solved[(1, 0)][0] == 0
        assert all((a, b) in known for a, b in solved)
    # test_ged_exact_host.py's admissibility check, on these graphs
    _admissible([ref.graph(a) for a in range(len(gs))], solved)


def test_sets_hold_what_the_issue_asks():
    n = {name: [g.number_of_nodes() for g in K.graphs(name)] for name in K.SETS}
    assert n['edge0'] == list(K.EDGE0_SIZES) and not any(g.number_of_edges() for g in K.graphs('edge0'))
    assert len({t for g in K.graphs('edge0') for t in nx.get_node_attributes(g, 'type').values()}) == 5
    fo = K.graphs('forest')
    assert min(n['forest']) == 4 and max(n['forest']) == 16
    for g in fo[:-1]:
        comps = sorted(len(c) for c in nx.connected_components(g))
        assert 2 <= len(comps) <= 4 and comps[0] == 1 and 2 in comps and nx.is_forest(g)
    assert sorted(d for _, d in fo[-1].degree()) == [1] * 16 and n['forest'][-1] == 16
    for g in K.graphs('dense') + K.graphs('densepm'):
        assert set(nx.get_node_attributes(g, 'type').values()) == {'C'}
    assert sorted({x[0] for x in K.DENSE['dense'] if not x[1]}) == [3, 9, 13, 16]
    assert (16, 8) in K.DENSE['densepm']
    t29 = K.graphs('types29')
    names = {t for g in t29 for t in nx.get_node_attributes(g, 'type').values()}
    assert names <= set(K.TYPES29) and len(K.TYPES29) == 29 and len(names) > 4
    assert min(n['types29']) == 2 and max(n['types29']) == 16
    distinct = [len(set(nx.get_node_attributes(g, 'type').values())) == g.number_of_nodes()
                for g in t29]
    assert distinct == [i % 2 == 0 for i in range(len(t29))]
    assert all(nx.is_connected(g) for g in t29)
    for name in ('forest', 'types29'):
        assert sum(1 for x in n[name] if x >= 13) >= 2 and 16 in n[name]
    big = [x for p in K.PLANTED for x in n[p]]
    assert sum(1 for x in big if x >= 13) >= 2 and 16 in big
    for p, N in zip(K.PLANTED, K.PLANTED_N):
        assert n[p] == [N] * 4 + [N + 1 if N < 16 else N - 1]
        assert all(nx.is_connected(g) for g in K.graphs(p))
    assert all(6 <= len(v) <= 10 or k in K.DENSE or k in K.PLANTED for k, v in n.items())


def test_the_proving_budget_is_rederived_and_within_the_cap(cache):
    """PROVE_BUDGET_WIDE is the smallest power of two at least twice the largest unlimited
    search of any within-set pair, and at most 2^18: a condition, not a measurement."""
    worst = max(v[3] for name in K.SETS for v in K.solved(name, cache).values())
    print('largest unlimited search: {} expansions'.format(worst))
    assert worst == K.MAX_PROVING_EXPANSIONS
    assert K.PROVE_BUDGET_WIDE == K.budget_for(worst)
    assert K.PROVE_BUDGET_WIDE >= 2 * worst > K.PROVE_BUDGET_WIDE // 2
    assert K.PROVE_BUDGET_WIDE <= K.BUDGET_CAP == 1 << 18 and K.PROVE_BUDGET_WIDE <= X.MAX_BUDGET
    assert worst > max(K.CUT_BUDGETS)            # the cut budgets of the GPU test do cut


def test_the_sets_reach_what_the_gpu_test_asserts(cache):
    """The pairs test_gpu_ged_classes.py's reach assertions need exist in the restatement."""
    reach = K.reach({name: K.solved(name, cache) for name in K.SETS})
    for what, pairs in reach.items():
        print(what, pairs[:3])
        assert pairs, what
