"""Maximum common induced subgraph on the device (include/siamese_mcs.h): a budgeted McSplit
search (McCreesh, Prosser, Trimble 2017) for every pair of a grid of store graphs in one call.

A common induced subgraph is an injective partial map of graph-1 nodes to graph-2 nodes of equal
`type` that keeps edges and non-edges; its size is the number of mapped nodes.  With connected
the mapped nodes must also induce a connected subgraph.  The search is cut off after `budget`
expansions per pair: where it finishes the size is proven (size == bound), elsewhere size is the
largest subgraph found and bound the root's upper bound.  The dense store serves graphs of at
most 32 nodes; a graph store (web.CsrStore) is refused.

This is the textbook problem.  It is not the connected maximum common edge subgraph over atom
and bond labels of the chorus library (MCS-DR) that the reference calls, and that program's
values are not claimed.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .ged import _index, _is_csr, store_of_graphs

MCS_DEFAULT_BUDGET = 1 << 20   # expansions per pair of distance.mcs


def mcs_grid(store, q_idx=None, db_idx=None, connected=False, budget=MCS_DEFAULT_BUDGET,
             bounds=False, edges=False, mapping=False, expansions=False, device='cuda', ld=None,
             return_status=False):
    """Maximum common induced subgraphs of store graphs q_idx x db_idx (None: every graph of the
    store), each search cut off after `budget` (an int in [0, 2^24]) expansions.

    Returns the size as a device int32 tensor [m][n]; with bounds=True (size, bound), proven
    where they are equal; with edges=True additionally the int32 tensor [m][n] of the edges of
    the subgraph found; with mapping=True the int8 tensor [m][n][n_max] of its map (-1: unmapped
    or beyond n1); with expansions=True the int64 tensor [m][n] of expansions spent, in this
    order.  A graph id outside the store or a node count outside [1, n_max] raises, unless
    return_status=True: then the int32 device status tensor [1] is returned last and such
    entries read -1.  ld > n gives the [m][n] outputs as [m][:n] views of [m][ld] buffers.

    A graph store (web.CsrStore) raises ValueError: the dense store only."""
    import torch
    if _is_csr(store):
        raise ValueError('the maximum common subgraph search serves the dense store only '
                         '(graphs of at most 32 nodes), not a graph store (CSR)')
    adj, types, n_nodes = store.to_device(device)
    G = int(n_nodes.numel())
    dev = adj.device
    q, db = _index(q_idx, dev), _index(db_idx, dev)
    m = G if q is None else int(q.numel())
    n = G if db is None else int(db.numel())
    ld = n if ld is None else int(ld)
    if ld < n:
        raise ValueError('ld {} below n {}'.format(ld, n))
    nbytes = _lib.mcs_grid_workspace_bytes(m, n, store.n_max)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=dev)
    size = torch.empty((m, ld), dtype=torch.int32, device=dev)
    bound = torch.empty((m, ld), dtype=torch.int32, device=dev)
    ed = torch.empty((m, ld), dtype=torch.int32, device=dev) if edges else None
    mp = torch.empty((m, n, store.n_max), dtype=torch.int8, device=dev) if mapping else None
    ex = torch.empty((m, ld), dtype=torch.int64, device=dev) if expansions else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.mcs_grid((adj, types, n_nodes), store.n_max, q, m, db, n, bool(connected), int(budget),
                  size, ld, bound, ed, mp, ex, status, ws)
    if not return_status:
        rc = int(status.item())
        if rc != 0:
            raise _lib.SiameseHipError('sg_mcs_grid: {} (a graph id outside the store, or a '
                                       'node count outside [1, n_max])'.format(
                                           _lib._ERR_NAMES.get(rc, rc)))
    out = [size[:, :n]]
    if bounds:
        out.append(bound[:, :n])
    if edges:
        out.append(ed[:, :n])
    if mapping:
        out.append(mp)
    if expansions:
        out.append(ex[:, :n])
    if return_status:
        out.append(status)
    return out[0] if len(out) == 1 else tuple(out)


def mcs_matrix(graphs_or_store, connected=False, budget=MCS_DEFAULT_BUDGET, device='cuda',
               node_feat_name='type'):
    """All-pairs sizes as a host int64 matrix [G][G] and the bool matrix of the pairs whose size
    the search proved.  networkx graphs go through ged.store_of_graphs, so a graph of more than
    32 nodes is refused as it is there."""
    store = graphs_or_store
    if not hasattr(store, 'to_device'):
        store = store_of_graphs(list(graphs_or_store), node_feat_name)
    size, bound = mcs_grid(store, connected=connected, budget=budget, bounds=True, device=device)
    size, bound = size.cpu().numpy().astype(np.int64), bound.cpu().numpy().astype(np.int64)
    return size, size == bound


def mcs_pair(g1, g2, connected=False, budget=MCS_DEFAULT_BUDGET, device='cuda',
             node_feat_name='type'):
    """(size, bound, edges) of two networkx graphs through a two-graph store; size == bound:
    proven."""
    store = store_of_graphs([g1, g2], node_feat_name)
    size, bound, ed = mcs_grid(store, [0], [1], connected=connected, budget=budget, bounds=True,
                               edges=True, device=device)
    return int(size.item()), int(bound.item()), int(ed.item())


def bunke_shearer(size, n):
    """The MCS metric of Bunke & Shearer 1998 as a float64 matrix: 1 - size[i][j] /
    max(n[i], n[j]) for the all-pairs sizes of graphs of n[i] nodes."""
    size = np.asarray(size, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64).reshape(-1)
    return 1.0 - size / np.maximum(n[:, None], n[None, :])
