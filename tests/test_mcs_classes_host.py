"""The sets of tests/_mcs_classes.py on the host: the restatement (tests/_mcs_restatement.py)
against the modular-product clique and the brute force of test_mcs_host.py, against the closed
forms and planted bounds of _mcs_classes.known, and as valid maps at every budget
test_gpu_mcs_classes.py uses.  Then what that test relies on: the budgets and the list of pairs
they leave unproven re-derived, the search's trace, and what the new sets reach that the four
sets of _mcs_cases.py do not.  No GPU."""
import networkx as nx
import pytest

import _ged_classes as K
import _mcs_cases as C
import _mcs_classes as M
import _mcs_restatement as X
from test_mcs_host import brute_force, check_map, modular_product_clique


def _cap(name):
    return M.DENSE_CAP if name in M.ALLOWED_UNPROVEN else None


def _allowed(name):
    return set(M.ALLOWED_UNPROVEN.get(name, ()))


def test_the_trace_changes_no_result():
    s, ref = C.store('one10')
    G = len(s)
    for connected in (False, True):
        for budget in (None, 7, 100):
            trace = {}
            for a in range(G):
                for b in range(G):
                    g1, g2 = ref.graph(a), ref.graph(b)
                    plain = X.search(g1, g2, connected, budget)
                    one = {}
                    assert X.search(g1, g2, connected, budget, trace=one) == plain
                    assert X.search(g1, g2, connected, budget, trace=trace) == plain
                    assert sorted(one) == sorted(X.TRACE_KEYS)
                    # one type: a class splits in two at most once per mapped node
                    assert one['classes_expanded'] <= s.n[a] and one['level'] < s.n[a]
                    assert not (one['no_class'] and not connected)
            if budget is None:
                assert trace['level'] > 0 and trace['classes_child'] >= 2
                assert (trace['no_class'] > 0) == connected


@pytest.mark.parametrize('name', M.SETS)
def test_budgets_and_the_unproven_list_rederive(name):
    """MAX_NEED is the largest proving need over the pairs the restatement proves (under
    DENSE_CAP on the dense sets, unlimited elsewhere), PROVE_BUDGET follows budget_for, and the
    pairs left unproven are ALLOWED_UNPROVEN exactly, at both `connected` values."""
    needs = M.proving_needs(name, _cap(name))
    unproven = {c: {(a, b) for (a, b, cc), (p, _) in needs.items() if cc == c and not p}
                for c in (0, 1)}
    assert unproven[0] == unproven[1] == _allowed(name)
    assert all(e == M.DENSE_CAP for p, e in needs.values() if not p)
    most = max(e for p, e in needs.values() if p)
    assert most == M.MAX_NEED[name]
    budget = M.PROVE_BUDGET[name]
    assert budget == K.budget_for(most) and budget & (budget - 1) == 0
    assert 2 * most <= budget < 4 * most and budget <= X.MAX_BUDGET
    assert M.budgets(name) == (0, 1, 7, budget)
    # at PROVE_BUDGET: the same pairs and no other
    s, ref = M.store(name)
    for c in (False, True):
        size, bound, _, _, ex = ref.grid(range(len(s)), range(len(s)), c, budget)
        left = {(a, b) for a in range(len(s)) for b in range(len(s)) if size[a, b] != bound[a, b]}
        assert left == _allowed(name)
        assert all(ex[a, b] == budget for a, b in left)
        assert max(ex[a, b] for a in range(len(s)) for b in range(len(s))
                   if (a, b) not in left) <= budget // 2


def test_the_sets_are_what_the_module_says():
    for name in M.SETS:
        s, _ = M.store(name)
        gs = M.graphs(name)
        assert s.n_max == M.capacity(name) and len(s) == len(gs)
        assert [int(x) for x in s.n[:len(gs)]] == [g.number_of_nodes() for g in gs]
    assert [g.number_of_nodes() for g in M.graphs('edge0')] == list(K.EDGE0_SIZES)
    for name in M.WIDE:
        g, pg, less, more = M.graphs(name)
        perm = M.permutation(name)
        assert [x.number_of_nodes() for x in (g, pg, less, more)] == [32, 32, 31, 32]
        assert K.is_isomorphism(g, pg, perm) and nx.is_connected(g)
        assert more.number_of_edges() == pg.number_of_edges() + 1
        assert set(pg.edges()) < set(more.edges())
        low = min(d for _, d in pg.degree())
        assert less.number_of_edges() == pg.number_of_edges() - low
        kinds = len(set(nx.get_node_attributes(g, 'type').values()))
        assert kinds == (32 if name == 'wide32' else M.WIDE_K8)
    a, b = M.graphs('wide32'), M.graphs('wide32k8')
    assert all(set(x.edges()) == set(y.edges()) for x, y in zip(a, b))
    for name in M.CAPS:
        gs = M.graphs(name)
        n = [g.number_of_nodes() for g in gs]
        assert 4 <= len(gs) <= 6 and 1 in n and M.capacity(name) in n
        assert len({t for g in gs for t in nx.get_node_attributes(g, 'type').values()}) == 2
    # the counted edits, from the graphs: relabels and edge edits against pi(g) on its nodes
    for name in K.PLANTED + M.WIDE:
        gs = M.graphs(name)
        pg = gs[1]
        edits = M.PLANTED_EDITS if name in K.PLANTED else M.WIDE_EDITS
        assert len(edits) == len(gs) and edits[:2] == (0, 0)
        for k in range(2, len(gs)):
            g = gs[k]
            if g.number_of_nodes() < pg.number_of_nodes():
                continue                              # renumbered: the restatement checks it
            n = pg.number_of_nodes()
            relabels = sum(1 for v in range(n) if g.nodes[v]['type'] != pg.nodes[v]['type'])
            e1 = {frozenset(e) for e in g.subgraph(range(n)).edges()}
            e0 = {frozenset(e) for e in pg.edges()}
            assert relabels + len(e1 ^ e0) == edits[k], (name, k)


@pytest.mark.parametrize('name', M.SETS)
def test_the_restatement_against_clique_brute_force_and_known(name):
    s, ref = M.store(name)
    G = len(s)
    gs = M.graphs(name)
    known = M.known(name)
    cap = _cap(name)
    n_clique = n_brute = n_known = 0
    res = {}
    for connected in (False, True):
        for a in range(G):
            for b in range(G):
                g1, g2 = ref.graph(a), ref.graph(b)
                size, bound, phi, edges, ex = ref.pair(a, b, connected, cap)
                proven = size == bound
                res[(a, b, connected)] = (size, proven)
                assert proven or (a, b) in _allowed(name)
                assert check_map(g1, g2, phi, connected) == (size, edges)
                small = max(s.n[a], s.n[b])
                if not connected and proven and small <= 10:
                    assert size == modular_product_clique(g1, g2), (a, b)
                    n_clique += 1
                if proven and small <= 6:
                    assert size == brute_force(g1, g2, connected), (a, b, connected)
                    n_brute += 1
                rule = known.get((a, b, int(connected)))
                if rule is not None:
                    assert M.holds(rule, size, proven), (a, b, connected, rule, size)
                    n_known += 1
                if name == 'edge0' and not connected:          # size = bound = ub0
                    assert size == bound == X._rest(X.root_classes(g1, g2)) == \
                        M.common_types(gs[a], gs[b])
                if (name in K.PLANTED or name in M.WIDE) and a < 2 and b < 2:
                    assert proven and size == s.n[a] and K.is_isomorphism(gs[a], gs[b], phi)
    for (a, b, connected), (size, proven) in res.items():
        back, bproven = res[(b, a, connected)]
        if proven and bproven:
            assert size == back, (a, b, connected)
        if connected and proven and res[(a, b, False)][1]:
            assert size <= res[(a, b, False)][0], (a, b)
    # every set is checked by something that is not the restatement
    assert n_known >= G
    if name in ('edge0', 'forest', 'types29', 'cap1', 'cap2', 'cap3'):
        assert n_brute >= 8
    assert n_clique >= sum(1 for g in gs if g.number_of_nodes() <= 10) ** 2
    if name in M.WIDE or name in K.PLANTED:
        assert sum(1 for r in known.values() if r[0] == 'ge') >= 6


@pytest.mark.parametrize('name', M.SETS)
def test_maps_are_common_induced_subgraphs_at_every_gpu_budget(name):
    s, ref = M.store(name)
    G = len(s)
    for budget in sorted(M.budgets(name), reverse=True):
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


def test_reach():
    """What makes the new sets worth their time, from the search's trace."""
    s, ref = M.store('wide32')
    one = {}
    proven, ex, ub0, _ = X.search(ref.graph(0), ref.graph(1), False, M.PROVE_BUDGET['wide32'],
                                  trace=one)
    assert proven and ex == 32 and ub0 == 32
    assert one['classes_expanded'] == 32 and one['level'] == 31       # in one search
    s, ref = M.store('wide32k8')
    wide = {}
    for a in range(len(s)):
        for b in range(len(s)):
            for connected in (False, True):
                X.search(ref.graph(a), ref.graph(b), connected, M.PROVE_BUDGET['wide32k8'],
                         trace=wide)
    assert wide['classes_expanded'] >= 16 and wide['classes_child'] >= 16
    s, ref = M.store('edge0')
    none = {}
    for a in range(len(s)):
        for b in range(len(s)):
            X.search(ref.graph(a), ref.graph(b), True, M.PROVE_BUDGET['edge0'], trace=none)
    assert none['no_class'] > 0
    # the four sets of _mcs_cases.py at their own budgets: at most 15 classes, which is the gap
    most = 0
    for name in C.NAMES:
        s, ref = C.store(name)
        budget = C.LARGE_BUDGET if name == 'two32' else C.PROVE_BUDGET
        old = {}
        for a in range(len(s)):
            for b in range(len(s)):
                for connected in (False, True):
                    X.search(ref.graph(a), ref.graph(b), connected, budget, trace=old)
        assert old['classes_expanded'] <= 15 and old['classes_child'] <= 15, name
        most = max(most, old['classes_expanded'])
    assert most == 15
