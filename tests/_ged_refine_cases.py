"""The graph sets and grids the GED refinement tests share (test_ged_refine_host.py derives on
the host what test_gpu_ged_refine.py relies on).  The stores b10 and b32 are _ged_beam_cases.py's,
by import; the restatement computes move costs incrementally, so both run whole (b32 with its
32 x 32 pairs in both orders) in a few seconds.

  r32   capacity 32: random connected graphs of (1, 7, 9, 8, 8, 5, 13, 32, 32) nodes over four
        types.  ROUNDS names the pairs with n1 * n2 = 1, 63, 64, 65 and 1024 moves: none, a
        partial round of the wavefront's 64 lanes, exactly one, one and one lane of a second,
        and all 16; every one but the first is refined (test_ged_refine_host.py).

BUDGETS[name] = (0, 1, M - 1, M, 4096) with M = MOST[name], the largest number of moves a single
start accepts on a pair of the set (test_ged_refine_host.py checks the figure).  GRIDS lists
(set, budgets, q ids, db ids; None: all graphs).
"""
import numpy as np

import _ged_beam_cases as BC
import _ged_exact_cases as C
import _ged_refine_restatement as F

SIZES = {'r32': (1, 7, 9, 8, 8, 5, 13, 32, 32)}
CAPACITY = {'b10': 10, 'b32': 32, 'r32': 32}
ROUNDS = {1: (0, 0), 63: (1, 2), 64: (3, 4), 65: (5, 6), 1024: (7, 8)}
MOST = {'b10': 4, 'b32': 15, 'r32': 17}
BUDGETS = {k: tuple(sorted({0, 1, m - 1, m, F.MAX_MOVES})) for k, m in MOST.items()}
GRIDS = tuple((name, BUDGETS[name], None, None) for name in ('b10', 'b32', 'r32'))

_GRAPHS = {}


def graphs(name):
    if name in BC.SIZES:
        return BC.graphs(name)
    if name not in _GRAPHS:
        rng = np.random.default_rng(411)
        _GRAPHS[name] = [C._random_graph(rng, n, i, p_extra=0.25)
                         for i, n in enumerate(SIZES[name])]
    return _GRAPHS[name]


_STORES = {}


def store(name):
    """(store, RefineGridReference) of a named set, built once per process."""
    if name not in _STORES:
        if name in BC.SIZES:
            s = BC.store(name)[0]
        else:
            from graphembedding_amd.ged import store_of_graphs
            s = store_of_graphs(graphs(name), n_max=CAPACITY[name])
        _STORES[name] = (s, F.RefineGridReference(s))
    return _STORES[name]


def ids(name, idx):
    return list(range(len(graphs(name)))) if idx is None else list(idx)
