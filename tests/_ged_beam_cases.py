"""The graph sets and grids the beam-search GED tests share (test_ged_beam_host.py derives on the
host what test_gpu_ged_beam.py relies on).  The generators are _ged_exact_cases.py's and
_ged_classes.py's, by import.

  b10   capacity 10: random connected graphs of (1, 2, 9, 10, 10, 9) nodes over four types, an
        edgeless graph of 7 nodes over five types, the one-type path, star (trees), cycle and
        complete graph on 6 nodes of _ged_exact_cases.graphs('tie10'), and a random connected
        graph of 8 nodes, all of different type, next to a permuted copy with one edge moved: the
        seed leaves ub 2 against lb 1, every level has one survivor and the last none, so even
        the width-1 beam runs to the end without a cut
  b32   capacity 32: random connected graphs of (1, 2, 16, 17, 31, 32, 32) nodes over four
        types, a one-type complete graph on 8 nodes, an edgeless graph of 32 nodes over five
        types, and a random connected graph of 32 nodes over 16 types (each twice) next to a copy
        of it under a node permutation with two edges moved: the seed leaves ub 4 against lb 3,
        so the pruning keeps the levels thin and all 32 levels run without a cut from width 63
        on.  Pairs come in both orders, so n2 + 1 = 33 children and n1 = 32 levels both occur.

GRIDS lists (set, widths, q ids, db ids; None: all graphs).  Every pair of b10 runs at every
width, which reaches the 63 / 64 / 65 states around the wavefront's 64 lanes; b32 runs whole at
the small widths and on a 3 x 5 grid of its large graphs at widths 65 and 128, which keeps the Python restatement's time for the whole list near a minute.
"""
import networkx as nx
import numpy as np

import _ged_beam_restatement as B
import _ged_classes as K
import _ged_exact_cases as C

WIDTHS = (0, 1, 2, 7, 63, 64, 65, 80, 128)
SMALL_WIDTHS = (0, 1, 2, 7)
SIZES = {'b10': (1, 2, 9, 10, 10, 9), 'b32': (1, 2, 16, 17, 31, 32, 32)}
CAPACITY = {'b10': 10, 'b32': 32}
GRIDS = (('b10', WIDTHS, None, None),
         ('b32', SMALL_WIDTHS, None, None),
         ('b32', (65, 128), (5, 3, 9), (4, 5, 6, 2, 10)))

_GRAPHS = {}


def graphs(name):
    if name not in _GRAPHS:
        rng = np.random.default_rng(('b10', 'b32').index(name) + 170)
        gs = [C._random_graph(rng, n, i, p_extra=0.15 if name == 'b10' else 0.08)
              for i, n in enumerate(SIZES[name])]
        if name == 'b10':
            gs.append(K._typed(nx.empty_graph(7), len(gs), K._draw(rng, K.TYPES5, 7)))
            for g in C.graphs('tie10'):
                gs.append(nx.Graph(g, gid=len(gs)))
            rng = np.random.default_rng(908)
            n = int(rng.integers(5, 10))
            g = C._random_graph(rng, n, len(gs), types=K.TYPES29[:n], p_extra=0.2)
            for v in range(n):
                g.nodes[v]['type'] = K.TYPES29[v]
            near = K._permuted(rng, g, len(gs) + 1)[0]
            gone = sorted(near.edges())[int(rng.integers(0, near.number_of_edges()))]
            new = sorted(nx.non_edges(near))
            near.remove_edge(*gone)
            near.add_edge(*new[int(rng.integers(0, len(new)))])
            gs += [g, near]
        else:
            gs.append(K._typed(nx.complete_graph(8), len(gs), ['C'] * 8))
            gs.append(K._typed(nx.empty_graph(32), len(gs), K._draw(rng, K.TYPES5, 32)))
            rng = np.random.default_rng(501)
            g = C._random_graph(rng, 32, len(gs), types=K.TYPES29, p_extra=0.08)
            for v in range(32):
                g.nodes[v]['type'] = K.TYPES29[v % 16]
            near = K._permuted(rng, g, len(gs) + 1)[0]
            for _ in range(2):
                gone = sorted(near.edges())[int(rng.integers(0, near.number_of_edges()))]
                new = sorted(nx.non_edges(near))[int(rng.integers(0, 100))]
                near.remove_edge(*gone)
                near.add_edge(*new)
            gs += [g, near]
        _GRAPHS[name] = gs
    return _GRAPHS[name]


_STORES = {}


def store(name):
    """(store, BeamGridReference) of a named set, built once per process."""
    if name not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        s = store_of_graphs(graphs(name), n_max=CAPACITY[name])
        _STORES[name] = (s, B.BeamGridReference(s))
    return _STORES[name]


def ids(name, idx):
    return list(range(len(graphs(name)))) if idx is None else list(idx)
