"""The restatement of include/siamese_mcs.h (tests/_mcs_restatement.py) against checks that do
not share its search: the largest clique of the modular product (networkx), a brute force over
all partial maps on the small graphs, and the properties every result must have.  Then the
conditions on the sets of tests/_mcs_cases.py that test_gpu_mcs.py relies on.  No GPU."""
import networkx as nx
import numpy as np
import pytest

import _mcs_cases as C
import _mcs_restatement as X


def _plain(g):
    """(types, set of ordered edges) of a restatement graph."""
    t, A = g
    n = len(t)
    return [int(x) for x in t], {(a, b) for a in range(n) for b in range(n) if A[a, b]}


def modular_product_clique(g1, g2):
    """The largest clique of the type-compatible modular product: nodes (a, b) of equal type,
    (a, b) ~ (c, d) iff a != c, b != d and (a, c) in E1 iff (b, d) in E2."""
    (t1, E1), (t2, E2) = _plain(g1), _plain(g2)
    nodes = [(a, b) for a in range(len(t1)) for b in range(len(t2)) if t1[a] == t2[b]]
    P = nx.Graph()
    P.add_nodes_from(nodes)
    for i, (a, b) in enumerate(nodes):
        for c, d in nodes[:i]:
            if a != c and b != d and ((a, c) in E1) == ((b, d) in E2):
                P.add_edge((a, b), (c, d))
    return max((len(c) for c in nx.find_cliques(P)), default=0)


def _connected(nodes, E):
    nodes = set(nodes)
    if not nodes:
        return True
    seen, todo = set(), [next(iter(nodes))]
    while todo:
        a = todo.pop()
        if a in seen:
            continue
        seen.add(a)
        todo.extend(b for b in nodes if (a, b) in E and b not in seen)
    return seen == nodes


def check_map(g1, g2, phi, connected):
    """phi is a common induced subgraph (connected where asked); returns (size, edges)."""
    (t1, E1), (t2, E2) = _plain(g1), _plain(g2)
    assert len(phi) == len(t1)
    mapped = [a for a, b in enumerate(phi) if b >= 0]
    img = [phi[a] for a in mapped]
    assert len(set(img)) == len(img) and all(0 <= b < len(t2) for b in img)
    for a in mapped:
        assert t1[a] == t2[phi[a]]
        for c in mapped:
            if a != c:
                assert ((a, c) in E1) == ((phi[a], phi[c]) in E2), (a, c)
    if connected:
        assert _connected(mapped, E1)
    return len(mapped), sum(1 for a in mapped for c in mapped if a < c and (a, c) in E1)


def brute_force(g1, g2, connected):
    """The largest common induced subgraph over all injective partial maps, node by node."""
    (t1, E1), (t2, E2) = _plain(g1), _plain(g2)
    n1, n2 = len(t1), len(t2)
    best = [0]

    def rec(a, phi):
        if a == n1:
            mapped = [x for x in range(n1) if phi[x] >= 0]
            if len(mapped) > best[0] and (not connected or _connected(mapped, E1)):
                best[0] = len(mapped)
            return
        rec(a + 1, phi + [-1])
        for b in range(n2):
            if b in phi or t1[a] != t2[b]:
                continue
            if all(((a, c) in E1) == ((b, phi[c]) in E2) for c in range(a) if phi[c] >= 0):
                rec(a + 1, phi + [b])

    rec(0, [])
    return best[0]


_ALL = {}


def _all_pairs(name, connected):
    """{(a, b): (size, bound, phi, edges, expansions)} with an unlimited budget."""
    if (name, connected) not in _ALL:
        s, ref = C.store(name)
        G = len(s)
        _ALL[(name, connected)] = {(a, b): ref.pair(a, b, connected, None)
                                   for a in range(G) for b in range(G)}
    return _ALL[(name, connected)]


@pytest.mark.parametrize('name', C.PROVEN_SETS)
def test_proven_sizes_equal_the_modular_product_clique(name):
    s, ref = C.store(name)
    res = _all_pairs(name, False)
    n_checked = 0
    for (a, b), r in res.items():
        assert r[0] == r[1]
        if max(s.n[a], s.n[b]) <= 10:
            assert r[0] == modular_product_clique(ref.graph(a), ref.graph(b)), (a, b)
            n_checked += 1
    assert n_checked >= {'one10': 36, 'tie6': 16, 'four10': 100}[name]


@pytest.mark.parametrize('connected', [False, True])
@pytest.mark.parametrize('name', C.PROVEN_SETS)
def test_small_pairs_equal_a_brute_force(name, connected):
    s, ref = C.store(name)
    res = _all_pairs(name, connected)
    n_checked = 0
    for (a, b), r in res.items():
        if max(s.n[a], s.n[b]) <= 6:
            assert r[0] == brute_force(ref.graph(a), ref.graph(b), connected), (a, b)
            n_checked += 1
    assert n_checked >= {'one10': 9, 'tie6': 16, 'four10': 36}[name]


def test_budgets_of_the_sets():
    """What test_gpu_mcs.py relies on: PROVE_BUDGET is the next power of two at or above twice
    the largest expansion count of the three proven sets, budgets 7 and 100 cut a one10 pair in
    mid-search, and two32 has a pair unproven at its largest budget."""
    most = max(max(C.proving_expansions(name).values()) for name in C.PROVEN_SETS)
    assert most <= C.PROVE_BUDGET // 2 and C.PROVE_BUDGET < 4 * most
    assert C.PROVE_BUDGET & (C.PROVE_BUDGET - 1) == 0 and C.PROVE_BUDGET <= X.MAX_BUDGET
    s, ref = C.store('one10')
    G = len(s)
    for budget in (7, 100):
        for connected in (False, True):
            cut = [ref.pair(a, b, connected, budget) for a in range(G) for b in range(G)]
            assert any(r[0] != r[1] and r[4] == budget for r in cut), (budget, connected)
    s, ref = C.store('two32')
    for connected in (False, True):
        size, bound, _, _, ex = ref.grid(range(len(s)), range(len(s)), connected, C.LARGE_BUDGET)
        assert (size != bound).any() and (ex[size != bound] == C.LARGE_BUDGET).all()
        assert (size <= bound).all()
    assert C.CUT_BUDGETS == (0, 1, 7, 100)


@pytest.mark.parametrize('name', C.NAMES)
def test_maps_are_common_induced_subgraphs_at_every_budget(name):
    s, ref = C.store(name)
    G = len(s)
    budgets = C.CUT_BUDGETS + ((C.LARGE_BUDGET,) if name == 'two32' else (C.PROVE_BUDGET,))
    for budget in budgets:
        sizes = {}
        for connected in (False, True):
            for a in range(G):
                for b in range(G):
                    g1, g2 = ref.graph(a), ref.graph(b)
                    size, bound, phi, edges, ex = ref.pair(a, b, connected, budget)
                    assert check_map(g1, g2, phi, connected) == (size, edges), (a, b)
                    ub0 = X._rest(X.root_classes(g1, g2))
                    assert 0 <= size <= bound <= ub0 and 0 <= ex <= budget
                    assert bound == (size if size == bound else ub0)
                    if budget == 0:
                        assert ex == 0 and size == 0 and (bound == 0) == (ub0 == 0)
                    sizes[(connected, a, b)] = (size, bound)
        if budget == C.PROVE_BUDGET:           # proven: the connected one is no larger
            for a in range(G):
                for b in range(G):
                    assert sizes[(True, a, b)][0] <= sizes[(False, a, b)][0]


@pytest.mark.parametrize('name', C.PROVEN_SETS)
def test_diagonal_symmetry_and_the_bunke_shearer_metric(name):
    from graphembedding_amd.mcs import bunke_shearer
    s, _ = C.store(name)
    G = len(s)
    for connected in (False, True):
        res = _all_pairs(name, connected)
        size = np.array([[res[(a, b)][0] for b in range(G)] for a in range(G)], dtype=np.int64)
        assert np.array_equal(np.diag(size), s.n[:G])        # the diagonal proves at n
        assert np.array_equal(size, size.T)
        if connected:
            continue
        d = bunke_shearer(size, s.n[:G])
        assert d.dtype == np.float64 and d.shape == (G, G) and not np.diag(d).any()
        assert (d >= 0).all() and (d <= 1).all()
        for i in range(G):
            for j in range(G):
                for k in range(G):
                    assert d[i, j] <= d[i, k] + d[k, j] + 1e-12, (i, j, k)
