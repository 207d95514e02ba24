"""Graph classes, capacities and a launch shape that _ged_beam_cases.py never gives the beam-search
GED (test_ged_beam_classes_host.py derives on the host what test_gpu_ged_beam_classes.py relies
on).  The generators are _ged_classes.py's and _ged_exact_cases.py's, by import.

  dense32    capacity 32, one type: K_32, K_32 minus the edge (3, 11), K_32 minus the perfect
             matching (2i, 2i+1), K_31, K_17, K_16 and K_9.  With K_32 minus a few edges as
             graph 2 the used-edge count EU of a state approaches 480 and costs reach 475, next
             to the type intersection at 32; every child of a level has almost the same f, so
             the selection orders thousands of candidates by index alone; and every mask has
             bit 31 set.  Closed forms: known_dense32
  edge0, forest, types29, planted16, planted9
             _ged_classes.py's sets at their own capacities (32 for edge0, else 16), with its
             oracles (edgeless_ged, known, is_isomorphism)
  cap1       capacity 1: four 1-node graphs over three types
  cap7       capacity 7: random connected graphs of (1, 2, 3, 5, 6, 7, 7) nodes over four
             types, the one-type cycle and complete graph on 7 nodes
  b10@c      the graphs of _ged_beam_cases.graphs('b10') stored at capacity c in RESTORED

GRIDS lists (set, widths); every grid is the whole set against itself.

NEVER_SEARCHED: three of these sets are not searched at any width, because the seed proves every
pair of them (test_ged_beam_classes_host.py asserts it): cap1, planted9, and edge0.  A pair with
an edgeless side never is: every node of the other graph is substituted or inserted, so its
degree is paid once under any assignment, the assignment problem minimises the type cost alone
and lb == ub.  These sets still run, for the seed path at their capacities, the closed forms
and the planted bounds; planted near-copies are searched in planted16.

BIG is a grid of more than 2^20 pairs over the b10 store: 1025 x 1024 ids drawn with a fixed
seed, every graph on both sides, so the launch has two grid rows and the second holds 1024 live
pairs.
"""
from math import comb

import networkx as nx
import numpy as np

import _ged_beam_cases as BC
import _ged_beam_restatement as B
import _ged_classes as K
import _ged_exact_cases as C

DENSE32 = ((32, 0), (32, 1), (32, 16), (31, 0), (17, 0), (16, 0), (9, 0))   # (n, edges K_n lacks)
DENSE32_WIDTHS = (1, 7, 64, 65, 128)
CLASS_WIDTHS = (1, 7, 128)
CLASS_SETS = ('edge0', 'forest', 'types29', 'planted16', 'planted9')
CAP7_SIZES = (1, 2, 3, 5, 6, 7, 7)
GRIDS = ((('dense32', DENSE32_WIDTHS),) + tuple((name, CLASS_WIDTHS) for name in CLASS_SETS) +
         (('cap1', CLASS_WIDTHS), ('cap7', CLASS_WIDTHS)))
SETS = tuple(name for name, _ in GRIDS)
NEVER_SEARCHED = ('edge0', 'planted9', 'cap1')      # the seed proves every pair of these
RESTORED = (16, 17, 31, 32)          # capacities the b10 graphs are stored at again
RESTORED_WIDTHS = (2, 80)

GRID_X = 1 << 20                     # pairs per grid row of the beam launch
BIG_M, BIG_N, BIG_LD, BIG_WIDTH, BIG_SEED = 1025, 1024, 1031, 1, 2048
BIG_LAST_Q = 3

_GRAPHS = {}


def _dense32():
    out = []
    for gid, (n, missing) in enumerate(DENSE32):
        g = nx.complete_graph(n)
        if missing == 16:
            g.remove_edges_from((2 * i, 2 * i + 1) for i in range(16))
        elif missing == 1:
            g.remove_edge(3, 11)
        out.append(K._typed(g, gid, ['C'] * n))
    return out


def graphs(name):
    if name not in _GRAPHS:
        if name == 'dense32':
            gs = _dense32()
        elif name in CLASS_SETS:
            gs = K.graphs(name)
        elif name == 'cap1':
            gs = [K._typed(nx.empty_graph(1), gid, [t]) for gid, t in enumerate('CNOC')]
        elif name == 'cap7':
            rng = np.random.default_rng(177)
            gs = [C._random_graph(rng, n, i, p_extra=0.2) for i, n in enumerate(CAP7_SIZES)]
            gs.append(K._typed(nx.cycle_graph(7), len(gs), ['C'] * 7))
            gs.append(K._typed(nx.complete_graph(7), len(gs), ['C'] * 7))
        else:
            raise KeyError(name)
        _GRAPHS[name] = gs
    return _GRAPHS[name]


def capacity(name):
    return {'dense32': 32, 'cap1': 1, 'cap7': 7}.get(name) or K.capacity(name)


_STORES = {}


def store(name):
    """(store, BeamGridReference) of a named set, built once per process."""
    if name not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        s = (K.store(name)[0] if name in CLASS_SETS
             else store_of_graphs(graphs(name), n_max=capacity(name)))
        assert s.n_max == capacity(name)
        _STORES[name] = (s, B.BeamGridReference(s))
    return _STORES[name]


def restored(c):
    """The b10 graphs in a store of capacity c."""
    if ('b10', c) not in _STORES:
        from graphembedding_amd.ged import store_of_graphs
        _STORES[('b10', c)] = store_of_graphs(BC.graphs('b10'), n_max=c)
    return _STORES[('b10', c)]


# ---- the oracles ----------------------------------------------------------------------------
def nearly_complete_ged32(a, missing):
    """K_a against K_32 minus `missing` disjoint edges: _ged_classes.nearly_complete_ged's
    argument at 32 nodes.  a nodes of the latter miss at least max(0, a - (32 - missing)) of
    those edges and a choice with exactly that many exists; every missing edge inside the image
    costs one edit, the 32 - a other nodes and every edge at them are inserted."""
    inside = max(0, a - (32 - missing))
    return (32 - a) + (comb(32, 2) - missing) - (comb(a, 2) - inside) + inside


def known_dense32():
    """{(a, b): GED} over the ordered pairs of dense32 that have a closed form: two complete
    graphs, or a complete graph against K_32 minus disjoint edges."""
    out = {}
    for a, (na, ma) in enumerate(DENSE32):
        for b, (nb, mb) in enumerate(DENSE32):
            if a == b:
                out[(a, b)] = 0
            elif ma == 0 and mb == 0:
                out[(a, b)] = K.complete_ged(na, nb)
            elif 0 in (ma, mb):
                out[(a, b)] = nearly_complete_ged32(min(na, nb), ma + mb)
    return out


def closed_form(name):
    """{(a, b): GED} of the pairs of dense32 or edge0 that have a closed form."""
    if name == 'dense32':
        return known_dense32()
    gs = graphs(name)
    return {(a, b): K.edgeless_ged(gs[a], gs[b])
            for a in range(len(gs)) for b in range(len(gs))}


# ---- the grid of more than 2^20 pairs -------------------------------------------------------
def big_ids():
    """(q [1025], db [1024]) ids into the b10 store: every graph first, then seeded draws, the
    whole under a seeded permutation; the last query, the one of the second grid row, is
    BIG_LAST_Q, a 10-node graph whose pairs are searched."""
    G = len(BC.graphs('b10'))
    rng = np.random.default_rng(BIG_SEED)
    out = []
    for size in (BIG_M, BIG_N):
        ids = np.concatenate([np.arange(G), rng.integers(0, G, size=size - G)])
        out.append(rng.permutation(ids).astype(np.int32))
    q, db = out
    at = int(np.flatnonzero(q == BIG_LAST_Q)[0])
    q[at], q[-1] = q[-1], q[at]
    return q, db


def grid_rows(m, n):
    """(gridDim.x, gridDim.y, live pairs of the last row) of the beam launch for m x n pairs."""
    pairs = m * n
    gx = min(pairs, GRID_X)
    gy = (pairs + gx - 1) // gx
    return gx, gy, pairs - (gy - 1) * gx
