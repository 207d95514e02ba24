"""Graph classes the GED tests of _ged_exact_cases.py never draw (test_ged_classes_host.py
proves on the host what test_gpu_ged_classes.py relies on), each a seeded set of networkx
graphs and a store through ged.store_of_graphs, with the oracles that need neither the
restatements nor networkx: closed forms and planted bounds.

  edge0      edgeless graphs of (1, 2, 5, 9, 13, 16, 17, 32) nodes, five types:
             GED = max(n1, n2) - |multiset intersection of the types|
  forest     an isolated node, a single edge and one or two random trees: 3 or 4 components,
             4 .. 16 nodes, each graph an induced subgraph of the next; then a perfect matching
             on 16 nodes; 16 type names, all distinct within a graph
  dense      one type: K_3, K_9, K_13, K_16 and K_16 minus one edge
  densepm    one type: K_3, K_16, K_16 minus a perfect matching, K_16 minus one edge.
             K_a against K_b, a <= b: (b - a) + C(b, 2) - C(a, 2); against K_16 minus disjoint
             edges: nearly_complete_ged.  K_16 minus a perfect matching is kept away from K_9
             and K_13: proving those two pairs takes the search more than 6 * 10^7 expansions
             (1.7 * 10^7 for K_9 as graph 1), above the call's limit of 2^24
  types29    29 type names, (2, 5, 8, 10, 13, 14, 16, 16) nodes: the first nodes of one
             _ged_exact_cases._random_graph, each under its own node permutation; in every
             other graph all types are distinct, in the rest some nodes repeat another's
  plantedN   N in (9, 12, 15, 16): a random connected g over 16 type names, pi(g) under a
             seeded permutation, and pi(g) after the first 1, 2 and 3 of: relabel one node;
             delete a non-bridge edge or add an edge; add a leaf (N < 16) or delete one (16).
             GED(g, pi(g)) = 0; GED is at most the cost of the edits between two of them, a relabel
             and an edge edit 1 each, a leaf 2 (its node and its edge)

The large graphs of forest, types29 and planted are alike and richly typed on purpose: the
depth-first search proves two unrelated 16-node graphs of four types only after millions of
expansions, and the Python restatement spends about 8000 expansions a second.

MAX_PROVING_EXPANSIONS is the largest expansion count the restatement needs with an unlimited
budget over the searched pairs (max(n1, n2) <= 16) within each set; PROVE_BUDGET_WIDE is the
smallest power of two at least twice it, the rule PROVE_BUDGET of _ged_exact_cases.py follows.
test_ged_classes_host.py re-derives both.
"""
import hashlib
import json
import os
from collections import Counter
from math import comb

import networkx as nx
import numpy as np

import _ged_exact_restatement as X
import _ged_restatement as R
from _ged_exact_cases import TYPES, _random_graph

TYPES5 = TYPES + ('P',)
TYPES29 = tuple('T{:02d}'.format(i) for i in range(29))
PLANTED_N = (9, 12, 15, 16)
PLANTED = tuple('planted{}'.format(n) for n in PLANTED_N)
SETS = ('edge0', 'forest', 'dense', 'densepm', 'types29') + PLANTED
EDGE0_SIZES = (1, 2, 5, 9, 13, 16, 17, 32)
TYPES29_SIZES = (2, 5, 8, 10, 13, 14, 16, 16)
DENSE = {'dense': ((3, 0), (9, 0), (13, 0), (16, 0), (16, 1)),       # (n, edges K_n lacks)
         'densepm': ((3, 0), (16, 0), (16, 8), (16, 1))}
CUT_BUDGETS = (0, 7, 1000)
# cost of the planted edits so far, by graph: a relabel 1, an edge 1, a leaf 2 (the node and its
# edge are one edit operation each in this cost model)
PLANTED_COST = (0, 0, 1, 2, 4)

MAX_PROVING_EXPANSIONS = 84780       # forest: 13 nodes against the perfect matching on 16
PROVE_BUDGET_WIDE = 1 << 18
BUDGET_CAP = 1 << 18


SEEDS = {'edge0': 700, 'forest': 731, 'dense': 0, 'densepm': 0, 'types29': 723, 'planted9': 724,
         'planted12': 725, 'planted15': 726, 'planted16': 727}


def _typed(g, gid, types):
    out = nx.Graph(gid=gid)
    for v in range(g.number_of_nodes()):
        out.add_node(v, type=types[v])
    out.add_edges_from(g.edges())
    return out


def _draw(rng, types, n):
    return [types[int(rng.integers(0, len(types)))] for _ in range(n)]


def _tree_edges(rng, s):
    """A random tree on 0 .. s-1 in which node 2i+1 hangs on node 2i: it holds a matching of
    all its nodes (but one, for odd s), so the forests stay near the perfect matching."""
    return [(i, i - 1 if i % 2 else int(rng.integers(0, i))) for i in range(1, s)]


FOREST_TREES = ((1, 0), (3, 0), (3, 3), (5, 3), (5, 5), (6, 5), (6, 7))


def _forest(rng):
    """An isolated node, a single edge and the first a and b nodes of two random trees (of 6
    and 7 nodes) per (a, b) of FOREST_TREES: 4 .. 16 nodes in 3 or 4 components, each graph an
    induced subgraph of the next so the large ones stay alike; then the perfect matching the
    last one nearly holds.  Every graph is put under its own node permutation."""
    names = [TYPES29[int(t)] for t in rng.permutation(29)[:16]]
    parts, base = [], 0
    for s in (1, 2, 6, 7):
        parts.append((s, _tree_edges(rng, s), names[base:base + s]))
        base += s
    plain = []
    for gid, (a, b) in enumerate(FOREST_TREES):
        g = nx.Graph(gid=gid)
        base = 0
        for (s, edges, names), take in zip(parts, (1, 2, a, b)):
            for v in range(take):
                g.add_node(base + v, type=names[v])
            g.add_edges_from((base + x, base + y) for x, y in edges if x < take and y < take)
            base += take
        assert 3 <= nx.number_connected_components(g) <= 4
        plain.append(g)
    # the matching: the single edge, the pairs of the two trees, and the isolated node with
    # the odd node of the 7-tree
    pm = nx.Graph(gid=len(plain))
    for v in range(16):
        pm.add_node(v, type=plain[-1].nodes[v]['type'])
    pm.add_edges_from([(0, 15)] + [(v, v + 1) for v in range(1, 15, 2)])
    plain.append(pm)
    return [_permuted(rng, g, gid)[0] for gid, g in enumerate(plain)]


def _dense(name):
    out = []
    for gid, (n, missing) in enumerate(DENSE[name]):
        g = nx.complete_graph(n)
        if missing == 8:
            g.remove_edges_from((2 * i, 2 * i + 1) for i in range(8))
        elif missing == 1:
            g.remove_edge(3, 11)
        out.append(_typed(g, gid, ['C'] * n))
    return out


def _permuted(rng, g, gid):
    """g under a seeded node permutation (node v becomes perm[v]), and perm."""
    n = g.number_of_nodes()
    perm = [int(x) for x in rng.permutation(n)]
    out = nx.Graph(gid=gid)
    for w in range(n):
        out.add_node(w, type=g.nodes[perm.index(w)]['type'])
    out.add_edges_from((perm[a], perm[b]) for a, b in g.edges())
    return out, perm


def _types29(rng):
    """Prefixes of one 16-node _random_graph (each is one itself), every graph under its own
    node permutation, so the large ones stay alike."""
    base = _random_graph(rng, 16, 0, types=TYPES29, p_extra=0.15)
    names = [TYPES29[int(t)] for t in rng.permutation(29)[:16]]
    out = []
    for gid, n in enumerate(TYPES29_SIZES):
        g = nx.Graph(base.subgraph(range(n)))
        for v in range(n):
            g.nodes[v]['type'] = names[v]        # all distinct
        if gid % 2:                              # repeats: some nodes take another node's name
            for v in rng.permutation(n)[:max(1, n // 8)]:
                g.nodes[int(v)]['type'] = names[(int(v) + 1 + int(rng.integers(0, n - 1))) % n]
        out.append(_permuted(rng, g, gid)[0])
    return out




def _planted(rng, n):
    types = TYPES29[:16]
    while True:
        g = _random_graph(rng, n, 0, types=types, p_extra=0.15)
        if n < 16 or sum(1 for v in g.nodes() if g.degree(v) == 1) >= 3:
            break
    pg, perm = _permuted(rng, g, 1)              # node v of g is node perm[v] of pi(g)
    out = [g, pg]
    cur = pg
    # 1: relabel one node
    cur = nx.Graph(cur, gid=2)
    v = int(rng.integers(0, n))
    other = [t for t in types if t != cur.nodes[v]['type']]
    cur.nodes[v]['type'] = other[int(rng.integers(0, len(other)))]
    out.append(cur)
    # 2: delete a non-bridge edge, or add an edge
    cur = nx.Graph(cur, gid=3)
    bridges = set(nx.bridges(cur))
    loose = sorted(e for e in cur.edges() if e not in bridges and e[::-1] not in bridges)
    if loose and n % 2:
        cur.remove_edge(*loose[int(rng.integers(0, len(loose)))])
    else:
        free = sorted(nx.non_edges(cur))
        cur.add_edge(*free[int(rng.integers(0, len(free)))])
    assert nx.is_connected(cur)
    out.append(cur)
    # 3: add a leaf, or at 16 nodes delete one
    if n < 16:
        cur = nx.Graph(cur, gid=4)
        cur.add_node(n, type=types[int(rng.integers(0, len(types)))])
        cur.add_edge(n, int(rng.integers(0, n)))
    else:
        leaves = [v for v in cur.nodes() if cur.degree(v) == 1]
        gone = leaves[int(rng.integers(0, len(leaves)))]
        keep = [v for v in range(n) if v != gone]
        nxt = nx.Graph(gid=4)
        for i, v in enumerate(keep):
            nxt.add_node(i, type=cur.nodes[v]['type'])
        nxt.add_edges_from((keep.index(a), keep.index(b)) for a, b in cur.edges()
                           if gone not in (a, b))
        cur = nxt
    out.append(cur)
    return out, perm


_GRAPHS = {}


def _build(name):
    rng = np.random.default_rng(SEEDS[name])
    if name == 'edge0':
        gs = []
        for gid, n in enumerate(EDGE0_SIZES):
            gs.append(_typed(nx.empty_graph(n), gid, _draw(rng, TYPES5, n)))
        return gs, None
    if name == 'forest':
        return _forest(rng), None
    if name in DENSE:
        return _dense(name), None
    if name == 'types29':
        return _types29(rng), None
    return _planted(rng, int(name[len('planted'):]))


def graphs(name):
    if name not in _GRAPHS:
        _GRAPHS[name] = _build(name)
    return _GRAPHS[name][0]


def permutation(name):
    """perm of a planted set: node v of graph 0 is node perm[v] of graph 1."""
    graphs(name)
    return _GRAPHS[name][1]


def capacity(name):
    return 32 if name == 'edge0' else 16


_STORES = {}


def store(name):
    """(store, GridReference, ExactGridReference) of a named set, built once per process."""
    if name not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        s = store_of_graphs(graphs(name), n_max=capacity(name))
        _STORES[name] = (s, R.GridReference(s), X.ExactGridReference(s))
    return _STORES[name]


# ---- the oracles ----------------------------------------------------------------------------
def edgeless_ged(g1, g2):
    t1 = Counter(nx.get_node_attributes(g1, 'type').values())
    t2 = Counter(nx.get_node_attributes(g2, 'type').values())
    return max(g1.number_of_nodes(), g2.number_of_nodes()) - sum((t1 & t2).values())


def complete_ged(a, b):
    a, b = min(a, b), max(a, b)
    return (b - a) + comb(b, 2) - comb(a, 2)


def nearly_complete_ged(a, missing):
    """K_a against K_16 minus `missing` disjoint edges (1: one edge, 8: a perfect matching).
    a nodes of the latter miss at least max(0, a - (16 - missing)) of those edges, and a choice
    with exactly that many exists; every missing edge inside the image costs one edit, the
    16 - a other nodes and every edge at them are inserted."""
    inside = max(0, a - (16 - missing))
    return (16 - a) + (comb(16, 2) - missing) - (comb(a, 2) - inside) + inside


def known(name):
    """{(a, b): ('eq' | 'le', value)} over ordered pairs of a set: what is known of GED(a, b)
    without a solver.  Pairs without an entry have no closed form."""
    gs = graphs(name)
    G = len(gs)
    out = {(a, a): ('eq', 0) for a in range(G)}
    if name == 'edge0':
        for a in range(G):
            for b in range(G):
                out[(a, b)] = ('eq', edgeless_ged(gs[a], gs[b]))
    elif name in DENSE:
        for a, (na, ma) in enumerate(DENSE[name]):
            for b, (nb, mb) in enumerate(DENSE[name]):
                if ma == 0 and mb == 0:
                    out[(a, b)] = ('eq', complete_ged(na, nb))
                elif 0 in (ma, mb):
                    out[(a, b)] = ('eq', nearly_complete_ged(min(na, nb), ma + mb))
    elif name in PLANTED:
        edits = PLANTED_COST
        for a in range(G):
            for b in range(G):
                if a != b:
                    d = abs(edits[a] - edits[b])
                    out[(a, b)] = ('eq', 0) if d == 0 else ('le', d)
    return out


def holds(rule, value):
    kind, v = rule
    return value == v if kind == 'eq' else value <= v


def searched_pairs(name):
    n = [g.number_of_nodes() for g in graphs(name)]
    return [(a, b) for a in range(len(n)) for b in range(len(n))
            if max(n[a], n[b]) <= X.MAX_SEARCH_NODES]


def is_isomorphism(g1, g2, phi):
    """phi (a list over the nodes of g1) maps g1 onto g2 keeping types and edges."""
    n = g1.number_of_nodes()
    if n != g2.number_of_nodes() or sorted(int(x) for x in phi[:n]) != list(range(n)):
        return False
    if any(g1.nodes[a]['type'] != g2.nodes[int(phi[a])]['type'] for a in range(n)):
        return False
    img = {frozenset((int(phi[a]), int(phi[b]))) for a, b in g1.edges()}
    return img == {frozenset(e) for e in g2.edges()}


# ---- the restatements over a set, cached ----------------------------------------------------
def _key(name):
    s = store(name)[0]
    h = hashlib.sha1(s.adj.tobytes() + s.types.tobytes() + s.n.tobytes())
    for mod in (R, X):
        with open(mod.__file__.replace('.pyc', '.py'), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


_SOLVED = {}


def solved(name, cache_dir):
    """{(a, b): (ub, lb, phi, expansions)} of the exact restatement with an unlimited budget
    over the searched ordered pairs of a set, cached as JSON under cache_dir (keyed by the
    set's arrays and the restatements' source)."""
    if name in _SOLVED:
        return _SOLVED[name]
    path = os.path.join(str(cache_dir), 'ged_classes_{}_{}.json'.format(name, _key(name)))
    if os.path.isfile(path):
        with open(path) as f:
            _SOLVED[name] = {tuple(int(x) for x in k.split(',')): (v[0], v[1], v[2], v[3])
                             for k, v in json.load(f).items()}
        return _SOLVED[name]
    ref = store(name)[2]
    out = {}
    for a, b in searched_pairs(name):
        ub, lb, phi, e = X.exact_pair(ref.graph(a), ref.graph(b), None)
        out[(a, b)] = (int(ub), int(lb), [int(x) for x in phi], int(e))
    with open(path, 'w') as f:
        json.dump({'{},{}'.format(*k): list(v) for k, v in out.items()}, f)
    _SOLVED[name] = out
    return out


def bp_ub(name):
    """{(a, b): the bipartite ub, the min over both orders} of the restatement."""
    ref = store(name)[1]
    return {(a, b): min(ref.pair(a, b)[0], ref.pair(b, a)[0]) for a, b in searched_pairs(name)}


def reach(results, bp=None):
    """The proven pairs with expansions > 0 that enter what _ged_exact_cases.py never proves,
    as {what: [(set, a, b)]}, from results {set: {(a, b): (ub, lb, map, expansions)}} and the
    bipartite ubs {set: {(a, b): ub}} (default: the restatement's)."""
    out = {'n1 = n2 = 16': [], 'n2 = 16 > n1 >= 9, nothing deleted': [],
           'n1 = 16 > n2 >= 9, a deletion': [], '9 <= n1, n2 <= 15': [],
           'ub below the bipartite ub at 13 or more nodes': []}
    for name, res in results.items():
        n = [g.number_of_nodes() for g in graphs(name)]
        ubs = bp_ub(name) if bp is None else bp[name]
        for (a, b), (ub, lb, phi, e) in res.items():
            if not (ub == lb and e > 0):
                continue
            n1, n2 = n[a], n[b]
            phi = [int(x) for x in phi[:n1]]
            if n1 == n2 == 16:
                out['n1 = n2 = 16'].append((name, a, b))
            if n2 == 16 > n1 >= 9 and -1 not in phi:
                out['n2 = 16 > n1 >= 9, nothing deleted'].append((name, a, b))
            if n1 == 16 > n2 >= 9 and -1 in phi:
                out['n1 = 16 > n2 >= 9, a deletion'].append((name, a, b))
            if 9 <= n1 <= 15 and 9 <= n2 <= 15:
                out['9 <= n1, n2 <= 15'].append((name, a, b))
            if min(n1, n2) >= 13 and ub < ubs[(a, b)]:
                out['ub below the bipartite ub at 13 or more nodes'].append((name, a, b))
    return out


def budget_for(max_expansions):
    """The smallest power of two at least twice max_expansions."""
    b = 1
    while b < 2 * max_expansions:
        b <<= 1
    return b
