"""The yardstick of the budgeted exact GED (tests/_ged_exact_restatement.py) against an
independent solver and against its own contract, on the host: with an unlimited budget it
equals networkx.graph_edit_distance, its map induces its ub, its h is admissible along optimal
paths, budget 0 is the bipartite seed, ub only falls and the proven set only grows with the
budget, and the set the GPU test expects proven is proven within half of that test's budget."""
import networkx as nx
import numpy as np
import pytest

import _ged_exact_cases as C
import _ged_exact_restatement as X
import _ged_restatement as R


def _random_connected(rng, n, n_types=3, p_extra=0.3):
    """test_ged_host.py's recipe."""
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
def graphs():
    """test_ged_host.py's 14 small graphs plus three 6-node ones: 289 ordered pairs, of which
    the 6-node ones against each other (the slowest for networkx) are 9."""
    rng = np.random.default_rng(20)
    gs = [_random_connected(rng, n) for n in (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 5)]
    return gs + [_random_connected(rng, 6, p_extra=p) for p in (0.1, 0.3, 0.5)]


@pytest.fixture(scope='module')
def solved(graphs):
    """{(i, j): (ub, lb, phi, expansions)} with an unlimited budget, for i <= j and for the
    pairs with a 6-node side in both orders (<= 250 pairs against networkx)."""
    G = len(graphs)
    out = {}
    for i in range(G):
        for j in range(G):
            if i <= j or max(i, j) >= G - 3:
                out[(i, j)] = X.exact_pair(graphs[i], graphs[j], None)
    assert len(out) <= 250
    return out


def test_unlimited_budget_equals_networkx(graphs, solved):
    for (i, j), (ub, lb, phi, _) in solved.items():
        assert ub == lb == _exact(graphs[i], graphs[j]), (i, j)


def test_map_induces_ub_and_is_a_partial_injection(graphs, solved):
    for (i, j), (ub, _, phi, _) in solved.items():
        g1, g2 = graphs[i], graphs[j]
        kept = [x for x in phi if x >= 0]
        assert len(phi) == len(g1[0]) and all(0 <= x < len(g2[0]) for x in kept)
        assert len(set(kept)) == len(kept)
        assert R.induced_cost(g1, g2, phi) == ub, (i, j)
    # also where the search is cut off, and at the seed itself (the inverse of the 2->1 map)
    n_inverse = 0
    for i, g1 in enumerate(graphs):
        for j, g2 in enumerate(graphs):
            for b in (0, 3):
                ub, lb, phi, e = X.exact_pair(g1, g2, b)
                assert R.induced_cost(g1, g2, phi) == ub and e <= b and lb <= ub
            n_inverse += R.upper_bound(g2, g1)[0] < R.upper_bound(g1, g2)[0]
    assert n_inverse > 0


def test_h_is_admissible_along_optimal_paths(graphs, solved):
    """Every node on the optimal path the search returned has g + h <= the optimum, h(root) is
    a lower bound, and h of a complete map is its leaf cost (f = the path's cost)."""
    for (i, j), (ub, _, phi, _) in solved.items():
        P = X._Pair(graphs[i], graphs[j])
        g, used = 0, 0
        assert P.h(0, 0) <= ub
        for k in range(P.n1):
            c = phi[k] if phi[k] >= 0 else P.n2
            g += P.step(phi[:k], c)
            if c < P.n2:
                used |= 1 << c
            assert g + P.h(k + 1, used) <= ub, (i, j, k)
        assert g + P.h(P.n1, used) == ub == R.induced_cost(graphs[i], graphs[j], phi)


def test_budget_zero_is_the_bipartite_seed(graphs):
    for g1 in graphs:
        for g2 in graphs:
            ub, lb, phi, e = X.exact_pair(g1, g2, 0)
            wub, wlb, _ = R.bp_pair(g1, g2, both_orders=True)
            assert (ub, lb, e) == (wub, wlb, 0)


def test_ub_falls_and_the_proven_set_grows_with_the_budget(graphs, solved):
    budgets = (0, 1, 7, 100, 10 ** 4)
    n_cut = 0
    for (i, j), full in solved.items():
        g1, g2 = graphs[i], graphs[j]
        seeded = X.seed(g1, g2)
        run = X.search(g1, g2, seeded[0], None)
        prev = None
        for b in budgets:
            got = X.exact_pair(g1, g2, b)
            # a smaller budget is a prefix of the same search (ExactGridReference relies on it)
            if X.searched(g1, g2, seeded[0], seeded[1], b):
                assert tuple(got) == tuple(X.at_budget(seeded, run, b)), (i, j, b)
            ub, lb, _, e = got
            assert e <= b and lb <= full[0] <= ub
            if prev is not None:
                assert ub <= prev[0] and lb >= prev[1] and e >= prev[3]
                assert not (prev[0] == prev[1]) or ub == lb        # proven stays proven
            n_cut += ub != lb
            prev = got
        assert tuple(prev) == tuple(full), (i, j)                   # 10^4 proves these all
    assert n_cut > 0


def test_skipped_above_sixteen_nodes():
    rng = np.random.default_rng(4)
    big, small = _random_connected(rng, 17, p_extra=0.05), _random_connected(rng, 3)
    for g1, g2 in ((big, small), (small, big), (big, big)):
        ub, lb, phi, e = X.exact_pair(g1, g2, 1000)
        assert (ub, lb, e) == R.bp_pair(g1, g2)[:2] + (0,)
        assert R.induced_cost(g1, g2, phi) == ub


@pytest.mark.parametrize('name', ['cap10', 'tie10'])
def test_gpu_proven_sets_need_at_most_half_the_gpu_budget(name, tmp_path_factory, request):
    """The GPU test passes C.PROVE_BUDGET and expects every pair of these sets proven: the
    restatement proves each within half of it, so no cut-off hides behind that budget."""
    cache = request.config.cache.mkdir('ged_exact') if hasattr(request.config, 'cache') \
        else tmp_path_factory.mktemp('ged_exact')
    exp = C.proving_expansions(name, cache)
    G = len(C.store(name)[0])
    assert len(exp) == G * G
    assert max(exp.values()) <= C.PROVE_BUDGET // 2, max(exp.values())
    assert C.PROVE_BUDGET <= X.MAX_BUDGET
    # the cut-off budgets of the GPU test do cut: some pair needs more than each of them
    assert max(exp.values()) > max(C.CUT_BUDGETS)
    assert any(v == 0 for v in exp.values()) and sum(1 for v in exp.values() if v) >= 4
