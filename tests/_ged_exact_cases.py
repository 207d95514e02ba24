"""The graph sets the exact-GED tests share (test_ged_exact_host.py proves on the host what
test_gpu_ged_exact.py relies on): random connected graphs drawn like test_gpu_ged.py's (a tree
plus extra edges, four types) and its tie-heavy single-type set.

  cap10  node counts (1, 2, 5, 8, 8, 7, 5, 2, 1, 8) in a capacity-10 store
  cap32  node counts (1, 8, 15, 16, 17, 32) in a capacity-32 store: the search limit at
         16 / 17 nodes and skipped pairs
  tie10  path, star, cycle and complete graph on 6 nodes, one type: every f ties

PROVE_BUDGET is the budget the GPU test passes to prove every pair of cap10 and tie10; the
host test shows the restatement needs at most half of it on each of them.
"""
import json
import os

import networkx as nx
import numpy as np

import _ged_exact_restatement as X

TYPES = ('C', 'N', 'O', 'S')
SIZES = {'cap10': (1, 2, 5, 8, 8, 7, 5, 2, 1, 8), 'cap32': (1, 8, 15, 16, 17, 32)}
PROVE_BUDGET = 1 << 15
CUT_BUDGETS = (0, 1, 7, 1000)


def _random_graph(rng, n, gid, types=TYPES, p_extra=0.15):
    g = nx.Graph(gid=gid)
    for v in range(n):
        g.add_node(v, type=types[int(rng.integers(0, len(types)))])
    for v in range(1, n):
        g.add_edge(v, int(rng.integers(0, v)))
    for a in range(n):
        for b in range(a):
            if rng.random() < p_extra:
                g.add_edge(a, b)
    return g


def graphs(name):
    rng = np.random.default_rng(('cap10', 'cap32', 'tie10').index(name) + 70)
    if name == 'tie10':
        gs = [nx.path_graph(6), nx.star_graph(5), nx.cycle_graph(6), nx.complete_graph(6)]
        out = []
        for i, g in enumerate(gs):
            g = nx.Graph(g, gid=i)
            nx.set_node_attributes(g, 'C', 'type')
            out.append(g)
        return out
    return [_random_graph(rng, n, i, p_extra=0.15 if name == 'cap10' else 0.08)
            for i, n in enumerate(SIZES[name])]


_STORES = {}


def store(name):
    """(store, ExactGridReference) of a named set, built once per process."""
    if name not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        s = store_of_graphs(graphs(name), n_max=32 if name == 'cap32' else 10)
        _STORES[name] = (s, X.ExactGridReference(s))
    return _STORES[name]


def proving_expansions(name, cache_dir):
    """{(a, b): expansions} of the restatement with an unlimited budget over all ordered pairs
    of a set, cached as JSON under cache_dir (keyed by the set's arrays)."""
    import hashlib
    s, ref = store(name)
    key = hashlib.sha1(s.adj.tobytes() + s.types.tobytes() + s.n.tobytes()).hexdigest()[:16]
    path = os.path.join(str(cache_dir), 'ged_exact_{}_{}.json'.format(name, key))
    if os.path.isfile(path):
        with open(path) as f:
            return {tuple(int(x) for x in k.split(',')): v for k, v in json.load(f).items()}
    G = len(s)
    out = {}
    for a in range(G):
        for b in range(G):
            g1, g2 = ref.graph(a), ref.graph(b)
            out[(a, b)] = X.exact_pair(g1, g2, None)[3]
    with open(path, 'w') as f:
        json.dump({'{},{}'.format(*k): v for k, v in out.items()}, f)
    return out
