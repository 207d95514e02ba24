"""Stores for the graph-store GED bounds that web.CsrStore never builds but
include/siamese_ged_csr.h permits (test_ged_csr_store_host.py derives on the host what
test_gpu_ged_csr_store.py relies on): rows without their diagonal entry, stored zeros, other
weights, types at the ends of [0, 2^22), and one-type graphs near K_300 whose CSR rows hold
hundreds of entries.

A variant is a copy of a CsrStore with row_ptr, col and val rebuilt from a per-graph pattern
(which entries are stored) and value matrix, row-major, so the columns of a row stay strictly
ascending; every edit here is symmetric.
"""
import copy

import networkx as nx
import numpy as np

from test_gpu_ged import _random_graph, _typed

SIZES = (1, 31, 33, 64, 65)
ISOLATED = (20, 2)                  # a random connected graph of 20 nodes and two isolated nodes
WEIGHT = 7.5
MAX_TYPE = (1 << 22) - 1            # the largest type the packed (type, degree) word holds
DENSE_N_MAX = 300
DENSE = ((300, 150), (290, 0), (257, 1))     # (n, disjoint edges K_n lacks)

_CACHE = {}


def graphs():
    if 'graphs' not in _CACHE:
        rng = np.random.default_rng(78)
        gs = [_random_graph(rng, n, i, p_extra=0.03) for i, n in enumerate(SIZES)]
        g = _random_graph(rng, ISOLATED[0], len(gs), p_extra=0.1)
        for v in range(ISOLATED[0], sum(ISOLATED)):
            g.add_node(v, type='N')
        gs.append(g)
        _CACHE['graphs'] = gs
    return _CACHE['graphs']


def base():
    if 'base' not in _CACHE:
        from graphembedding_amd.ged import csr_store_of_graphs
        _CACHE['base'] = csr_store_of_graphs(graphs())
    return _CACHE['base']


def dense_of(store, g):
    """(pattern bool [n][n], values float32 [n][n]) of store graph g."""
    off, n = int(store.node_off[g]), int(store.n[g])
    P = np.zeros((n, n), dtype=bool)
    V = np.zeros((n, n), dtype=np.float32)
    for a in range(n):
        s0, s1 = int(store.row_ptr[off + a]), int(store.row_ptr[off + a + 1])
        P[a, store.col[s0:s1]] = True
        V[a, store.col[s0:s1]] = store.val[s0:s1]
    return P, V


def rebuilt(store, mats):
    """A copy of store with the CSR arrays of mats = [(pattern, values)] by graph."""
    out = copy.copy(store)
    row_ptr, cols, vals, nnz = [np.zeros(1, dtype=np.int64)], [], [], 0
    for g, (P, V) in enumerate(mats):
        assert P.shape == (int(store.n[g]),) * 2 and np.array_equal(P, P.T)
        r, c = np.nonzero(P)                              # row-major: columns ascending
        row_ptr.append(nnz + np.cumsum(np.bincount(r, minlength=P.shape[0])))
        cols.append(c.astype(np.int32))
        vals.append(V[r, c].astype(np.float32))
        nnz += r.size
    out.row_ptr = np.concatenate(row_ptr).astype(np.int32)
    out.col = np.concatenate(cols)
    out.val = np.concatenate(vals)
    out.types = store.types.copy()
    out.max_nnz = int(np.diff(out.row_ptr[out.node_off]).max())
    out._dev = out._struct = None
    return out


def _edges(P, V):
    """The edges (a < b) of a graph: stored, off the diagonal, non-zero."""
    a, b = np.nonzero(np.triu(P & (V != 0), 1))
    return list(zip(a.tolist(), b.tolist()))


def zeroed_edges():
    """By graph of graphs(): the seeded set of real edges variant (d) turns into stored zeros
    (a third of them, at least one where the graph has an edge)."""
    rng = np.random.default_rng(79)
    out = []
    for g in graphs():
        es = sorted(tuple(sorted(e)) for e in g.edges())
        k = min(len(es), max(1, len(es) // 3))
        out.append([es[int(i)] for i in rng.permutation(len(es))[:k]])
    return out


def variants():
    """{name: store}: 'nodiag' (a), 'scaled' (b), 'zeros_added' (c), 'zeros_for_edges' (d) and
    'edges_removed': the store web.CsrStore builds of the graphs without the edges of (d)."""
    if 'variants' in _CACHE:
        return _CACHE['variants']
    from graphembedding_amd.ged import csr_store_of_graphs
    s = base()
    G = len(s)
    mats = [dense_of(s, g) for g in range(G)]
    out = {}
    out['nodiag'] = rebuilt(s, [(P & ~np.eye(len(P), dtype=bool), V) for P, V in mats])
    out['scaled'] = rebuilt(s, [(P, V * np.float32(WEIGHT)) for P, V in mats])
    rng = np.random.default_rng(80)
    added = []
    for P, V in mats:
        free = [(a, b) for a in range(len(P)) for b in range(a + 1, len(P)) if not P[a, b]]
        k = min(len(free), len(_edges(P, V)) // 3)
        P = P.copy()
        for i in rng.permutation(len(free))[:k]:
            a, b = free[int(i)]
            P[a, b] = P[b, a] = True                      # V stays 0 there
        added.append((P, V))
    out['zeros_added'] = rebuilt(s, added)
    zeroed, removed = [], []
    for (P, V), g, gone in zip(mats, graphs(), zeroed_edges()):
        V = V.copy()
        h = nx.Graph(g)
        for a, b in gone:
            V[a, b] = V[b, a] = 0
            h.remove_edge(a, b)
        zeroed.append((P, V))
        removed.append(h)
    out['zeros_for_edges'] = rebuilt(s, zeroed)
    out['edges_removed'] = csr_store_of_graphs(removed)
    _CACHE['variants'] = out
    return out


def retyped(store, changes):
    """A copy of store with types[node_off[g] + a] = t for every (g, a, t)."""
    out = copy.copy(store)
    out.types = store.types.copy()
    for g, a, t in changes:
        out.types[int(store.node_off[g]) + a] = t
    out._dev = out._struct = None
    return out


def dense_graphs():
    """One type: K_300 minus the perfect matching (2i, 2i+1), K_290, K_257 minus the edge
    (3, 11)."""
    out = []
    for gid, (n, missing) in enumerate(DENSE):
        g = nx.complete_graph(n)
        if missing == 1:
            g.remove_edge(3, 11)
        elif missing:
            g.remove_edges_from((2 * i, 2 * i + 1) for i in range(missing))
        out.append(_typed(g, gid))
    return out


def dense_store():
    if 'dense' not in _CACHE:
        from graphembedding_amd.ged import csr_store_of_graphs
        _CACHE['dense'] = csr_store_of_graphs(dense_graphs())
    return _CACHE['dense']
