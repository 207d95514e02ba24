"""The graph sets the MCS tests share (test_mcs_host.py proves on the host what test_gpu_mcs.py
relies on): random connected graphs drawn as _ged_exact_cases._random_graph draws them.  With
four types the search proves a 10-node pair in a few dozen expansions, so the sets that budgets
are to cut have one or two types.

  one10   one type, node counts (1, 2, 6, 8, 10, 10, 12) in a capacity-32 store: every pair
          is proven within PROVE_BUDGET
  two32   two types, node counts (1, 10, 16, 24, 32, 32) in a capacity-32 store: the large
          case, cut off by every budget the tests use
  tie6    path, star, cycle and complete graph on 6 nodes, one type, capacity 10: every
          max(|L|, |R|) ties
  four10  the exact-GED cap10 recipe (four types) in a capacity-10 store: type splitting and
          pairs with few or no common types

PROVE_BUDGET is the budget the GPU test passes to prove every pair of one10, tie6 and four10 at
both `connected` values: the next power of two at or above twice the largest expansion count
the restatement needs on them with an unlimited budget (318, measured on the host with
tests/_mcs_restatement.py; test_mcs_host.py asserts the factor two).
"""
import networkx as nx
import numpy as np

import _mcs_restatement as X
from _ged_exact_cases import _random_graph

TYPES = ('C', 'N', 'O', 'S')
SIZES = {'one10': (1, 2, 6, 8, 10, 10, 12), 'two32': (1, 10, 16, 24, 32, 32),
         'four10': (1, 2, 5, 8, 8, 7, 5, 2, 1, 8)}
N_TYPES = {'one10': 1, 'two32': 2, 'four10': 4}
P_EXTRA = {'one10': 0.15, 'two32': 0.08, 'four10': 0.15}
N_MAX = {'one10': 32, 'two32': 32, 'tie6': 10, 'four10': 10}
SEEDS = {'one10': 90, 'two32': 91, 'four10': 92}
NAMES = ('one10', 'two32', 'tie6', 'four10')
PROVEN_SETS = ('one10', 'tie6', 'four10')
PROVE_BUDGET = 1 << 10
CUT_BUDGETS = (0, 1, 7, 100)
LARGE_BUDGET = 1000            # two32's largest


def graphs(name):
    if name == 'tie6':
        gs = [nx.path_graph(6), nx.star_graph(5), nx.cycle_graph(6), nx.complete_graph(6)]
        out = []
        for i, g in enumerate(gs):
            g = nx.Graph(g, gid=i)
            nx.set_node_attributes(g, 'C', 'type')
            out.append(g)
        return out
    rng = np.random.default_rng(SEEDS[name])
    return [_random_graph(rng, n, i, types=TYPES[:N_TYPES[name]], p_extra=P_EXTRA[name])
            for i, n in enumerate(SIZES[name])]


_STORES = {}


def store(name):
    """(store, McsGridReference) of a named set, built once per process."""
    if name not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        s = store_of_graphs(graphs(name), n_max=N_MAX[name])
        _STORES[name] = (s, X.McsGridReference(s))
    return _STORES[name]


def proving_expansions(name):
    """{(a, b, connected): expansions} of the restatement with an unlimited budget over all
    ordered pairs of a set and both `connected` values."""
    s, ref = store(name)
    G = len(s)
    return {(a, b, c): ref.pair(a, b, bool(c), None)[4]
            for a in range(G) for b in range(G) for c in (0, 1)}
