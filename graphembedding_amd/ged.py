"""Graph edit distance on the device (include/siamese_ged.h): the bipartite approximation of
Riesen & Bunke for every pair of a grid of store graphs in one call, with the certified lower
bound of the same construction.

Cost model (the graph-matching-toolkit's for the AIDS sets, doubled at alpha = 0.5): node
insertion / deletion 1, node substitution 0 for equal `type` and 1 otherwise, edge insertion /
deletion 1, edge substitution 0.  lb <= GED <= ub; where lb == ub the distance is exact.  The
dense store serves graphs of at most 32 nodes (capacities 10 and 32); a graph store (web.CsrStore,
csr_store_of_graphs) serves graphs of at most 512 nodes through include/siamese_ged_csr.h, with
the same construction and tie rules, bounds only.

With exact_budget the calls go through include/siamese_ged_exact.h instead: a depth-first branch
and bound per pair, seeded with those bounds and cut off after exact_budget expansions.  It
proves the distance (lb == ub) where it finishes, which it does on graphs of at most about 10
nodes, and tightens ub elsewhere; graphs of more than 16 nodes keep the bipartite bounds.

With beam_width the calls go through include/siamese_ged_beam.h: a level-synchronous beam of at
most beam_width states per pair, seeded with the same bounds, for every graph of the store (no
16-node limit).  It tightens ub, and proves the distance (lb == ub) where the width never cut a
level.  It is not the graph-matching-toolkit's beam search and does not claim its values.

With refine_moves the calls go through include/siamese_ged_refine.h: local search on the node
map, the 2-exchange refinement (K-REFINE with K = 2) of both bipartite maps, of at most
refine_moves accepted moves per start, for every graph of the store.  It tightens ub and proves
nothing by itself: lb stays the bipartite one.

ged_knn is the query on top of the bounds and the exact search (include/siamese_ged_knn.h): the
k nearest database graphs of every query under exact GED, by filter and verify.  The k-th
smallest upper bound of a row is its threshold; a pair whose lower bound exceeds it is never
searched, and every other pair is searched from the threshold instead of its own upper bound, so
a pair that only has to be shown farther than the threshold is cut off early.  A certified row
is the true top-k in ascending (distance, column); knn_recall scores any other top-k (a learned
index's `nearest`) against it.
"""
from __future__ import annotations

import numpy as np

from . import _lib

GED_MAX_NODES = 32
GED_CSR_MAX_NODES = 512              # graph-store (CSR) graphs: the bipartite bounds only
GED_EXACT_MAX_NODES = 16             # larger graphs keep the bipartite bounds
GED_EXACT_DEFAULT_BUDGET = 1 << 20   # expansions per pair of distance.ged(..., 'exact')
GED_BEAM_DEFAULT_WIDTH = 80          # states per level of beam_label_matrix
GED_REFINE_DEFAULT_MOVES = 1024      # accepted moves per start of refine_label_matrix


def _index(idx, device):
    import torch
    if idx is None:
        return None
    return torch.as_tensor(idx, dtype=torch.int32, device=device).reshape(-1).contiguous()


def ged_grid(store, q_idx=None, db_idx=None, both_orders=True, bounds=False, mapping=False,
             device='cuda', ld=None, return_status=False, exact_budget=None, expansions=False,
             beam_width=None, expanded=False, refine_moves=None, moves=False):
    """Bipartite GED bounds of store graphs q_idx x db_idx (None: every graph of the store).

    Returns the upper bound ub as a device int32 tensor [m][n] (min over both assignment
    orders with both_orders); with bounds=True (ub, lb); with mapping=True additionally the
    int8 tensor [m][n][n_max] of the 1->2 assignment (-1: deleted or beyond n1).  A graph id
    outside the store or a node count outside [1, n_max] raises, unless return_status=True:
    then the int32 device status tensor [1] is returned last and such entries read -1.
    ld > n gives ub / lb as [m][:n] views of [m][ld] buffers.

    exact_budget=B (an int in [0, 2^24]) runs the budgeted branch and bound on every pair: ub is
    the cost of the best edit path found (never above the bipartite one), lb equals ub where the
    distance is proven, the mapping is that path's, and expansions=True additionally returns the
    int64 tensor [m][n] of expansions spent (after the mapping, before the status).

    beam_width=w (an int in [0, 128]; not together with exact_budget) runs the level-synchronous
    beam on every pair instead and returns (ub, lb, ...) in the same way: lb equals ub where the
    beam was never truncated, and expanded=True additionally returns the int32 tensor [m][n] of
    states expanded, in the place expansions takes.

    refine_moves=k (an int in [0, 4096]; not together with exact_budget or beam_width) runs the
    2-exchange refinement of both bipartite maps on every pair instead, at most k accepted moves
    per start, and returns (ub, lb, ...) in the same way: lb is the bipartite one, and moves=True
    additionally returns the int32 tensor [m][n] of moves accepted, in the place expanded takes.

    A graph store (web.CsrStore) goes through sg_csr_ged_grid: the same bounds for graphs of at
    most 512 nodes, the mapping an int16 tensor; exact_budget, beam_width and refine_moves raise
    ValueError there."""
    import torch
    if _is_csr(store):
        if (exact_budget is not None or beam_width is not None or refine_moves is not None
                or expansions or expanded or moves):
            raise ValueError('a graph store (CSR) has the bipartite bounds only: no exact_budget, '
                             'no beam_width, no refine_moves')
        return _csr_ged_grid(store, q_idx, db_idx, both_orders, bounds, mapping, device, ld,
                             return_status)
    exact = exact_budget is not None
    beam = beam_width is not None
    refine = refine_moves is not None
    if exact + beam + refine > 1:
        raise ValueError('exact_budget, beam_width and refine_moves are mutually exclusive')
    if expansions and not exact:
        raise ValueError('expansions are counted by the exact search: pass exact_budget')
    if expanded and not beam:
        raise ValueError('expanded states are counted by the beam search: pass beam_width')
    if moves and not refine:
        raise ValueError('moves are counted by the refinement: pass refine_moves')
    if exact and not both_orders:
        raise ValueError('the exact search is seeded with both assignment orders')
    if beam and not both_orders:
        raise ValueError('the beam search is seeded with both assignment orders')
    if refine and not both_orders:
        raise ValueError('the refinement starts from both assignment orders')
    adj, types, n_nodes = store.to_device(device)
    G = int(n_nodes.numel())
    dev = adj.device
    q, db = _index(q_idx, dev), _index(db_idx, dev)
    m = G if q is None else int(q.numel())
    n = G if db is None else int(db.numel())
    ld = n if ld is None else int(ld)
    if ld < n:
        raise ValueError('ld {} below n {}'.format(ld, n))
    nbytes = (_lib.ged_exact_grid_workspace_bytes if exact else
              _lib.ged_beam_grid_workspace_bytes if beam else
              _lib.ged_refine_grid_workspace_bytes if refine else
              _lib.ged_grid_workspace_bytes)(m, n, store.n_max)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=dev)
    ub = torch.empty((m, ld), dtype=torch.int32, device=dev)
    lb = torch.empty((m, ld), dtype=torch.int32, device=dev) if bounds or exact or beam or refine else None
    mp = torch.empty((m, n, store.n_max), dtype=torch.int8, device=dev) if mapping else None
    ex = torch.empty((m, ld), dtype=torch.int64, device=dev) if expansions else None
    if expanded or moves:
        ex = torch.empty((m, ld), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if exact:
        _lib.ged_exact_grid((adj, types, n_nodes), store.n_max, q, m, db, n, int(exact_budget),
                            ub, ld, lb, mp, ex, status, ws)
    elif beam:
        _lib.ged_beam_grid((adj, types, n_nodes), store.n_max, q, m, db, n, int(beam_width),
                           ub, ld, lb, mp, ex, status, ws)
    elif refine:
        _lib.ged_refine_grid((adj, types, n_nodes), store.n_max, q, m, db, n, int(refine_moves),
                             ub, ld, lb, mp, ex, status, ws)
    else:
        _lib.ged_grid((adj, types, n_nodes), store.n_max, q, m, db, n, both_orders, ub, ld, lb,
                      mp, status, ws)
    if not return_status:
        rc = int(status.item())
        if rc != 0:
            raise _lib.SiameseHipError('{}: {} (a graph id outside the store, or a '
                                       'node count outside [1, n_max])'.format(
                                           'sg_ged_exact_grid' if exact else
                                           'sg_ged_beam_grid' if beam else
                                           'sg_ged_refine_grid' if refine else 'sg_ged_grid',
                                           _lib._ERR_NAMES.get(rc, rc)))
    out = [ub[:, :n]]
    if bounds:
        out.append(lb[:, :n])
    if mapping:
        out.append(mp)
    if expansions or expanded or moves:
        out.append(ex[:, :n])
    if return_status:
        out.append(status)
    return out[0] if len(out) == 1 else tuple(out)


def ged_knn(store, q_idx=None, db_idx=None, k=10, exact_budget=GED_EXACT_DEFAULT_BUDGET,
            device='cuda', stats=False, return_status=False):
    """The k nearest graphs db_idx of every query q_idx of a dense store under exact GED (None:
    every graph of the store), by sg_ged_knn: filter by the bipartite bounds, verify under the
    row's threshold with at most exact_budget expansions per pair.

    Returns (cols, ub, lb, certified) as device int32 tensors: cols [m][k] the columns (indices
    into db_idx) in ascending (ub, column), ub / lb [m][k] their bounds (lb == ub: proven),
    certified [m] 1 where the row is proven to be the true top-k of the exact distances in
    ascending (distance, column).  With fewer than k servable database graphs the last slots
    read -1.  stats=True additionally returns candidates (int32 [m], the pairs that survived
    the filter) and expansions (int64 [m], summed over the row).  A graph id outside the store
    or a node count outside [1, n_max] raises, unless return_status=True: then the int32 device
    status tensor [1] is returned last, such a query's row reads -1 with certified 0 and such a
    database graph takes no part.  A graph store (web.CsrStore) raises ValueError."""
    import torch
    if _is_csr(store):
        raise ValueError('a graph store (CSR) has the bipartite bounds only: no ged_knn')
    k = int(k)
    if not 1 <= k <= _lib.GED_KNN_MAX_K:
        raise ValueError('k {} outside [1, {}]'.format(k, _lib.GED_KNN_MAX_K))
    budget = int(exact_budget)
    if not 0 <= budget <= _lib.GED_EXACT_MAX_BUDGET:
        raise ValueError('exact_budget {} outside [0, {}]'.format(
            budget, _lib.GED_EXACT_MAX_BUDGET))
    adj, types, n_nodes = store.to_device(device)
    G = int(n_nodes.numel())
    dev = adj.device
    q, db = _index(q_idx, dev), _index(db_idx, dev)
    m = G if q is None else int(q.numel())
    n = G if db is None else int(db.numel())
    nbytes = _lib.ged_knn_workspace_bytes(m, n, store.n_max, k)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)   # 8-byte aligned
    cols = torch.empty((m, k), dtype=torch.int32, device=dev)
    ub = torch.empty((m, k), dtype=torch.int32, device=dev)
    lb = torch.empty((m, k), dtype=torch.int32, device=dev)
    cert = torch.empty((m,), dtype=torch.int32, device=dev)
    cand = torch.empty((m,), dtype=torch.int32, device=dev) if stats else None
    ex = torch.empty((m,), dtype=torch.int64, device=dev) if stats else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.ged_knn((adj, types, n_nodes), store.n_max, q, m, db, n, k, budget, cols, ub, lb, cert,
                 cand, ex, status, ws)
    if not return_status:
        rc = int(status.item())
        if rc != 0:
            raise _lib.SiameseHipError('sg_ged_knn: {} (a graph id outside the store, or a '
                                       'node count outside [1, n_max])'.format(
                                           _lib._ERR_NAMES.get(rc, rc)))
    out = [cols, ub, lb, cert]
    if stats:
        out += [cand, ex]
    if return_status:
        out.append(status)
    return tuple(out)


def ged_knn_graphs(graphs, queries, k=10, exact_budget=GED_EXACT_DEFAULT_BUDGET, device='cuda',
                   node_feat_name='type'):
    """ged_knn for networkx graphs, in the manner of ged_matrix: the k nearest of `graphs` for
    every graph of `queries` as host arrays (cols int64 [m][k] indices into graphs, dist int64
    [m][k] the ub, proven bool [m][k], certified bool [m]).  Both lists go into one store, so
    their types are encoded together; graphs of at most 32 nodes."""
    graphs, queries = list(graphs), list(queries)
    store = store_of_graphs(graphs + queries, node_feat_name)
    n = len(graphs)
    cols, ub, lb, cert = ged_knn(store, np.arange(n, n + len(queries)), np.arange(n), k=k,
                                 exact_budget=exact_budget, device=device)
    ub, lb = ub.cpu().numpy().astype(np.int64), lb.cpu().numpy().astype(np.int64)
    return cols.cpu().numpy().astype(np.int64), ub, (ub == lb) & (ub >= 0), \
        cert.cpu().numpy().astype(bool)


def knn_recall(pred_cols, true_cols, certified):
    """(recall, rows): the mean over the certified rows of |pred ∩ true| / k', k' the number of
    entries >= 0 of the row of true_cols (ged_knn's cols), and the number of rows counted.
    pred_cols is any [m][k_pred] top-k of the same queries against the same database (entries
    < 0 are ignored), e.g. EmbeddingIndex.nearest's; rows that are not certified or have no
    true neighbour are left out, and with no row counted the recall is nan."""
    pred = _host(pred_cols)
    true = _host(true_cols)
    cert = _host(certified).astype(bool).reshape(-1)
    if pred.ndim != 2 or true.ndim != 2 or not pred.shape[0] == true.shape[0] == cert.shape[0]:
        raise ValueError('pred_cols [m][k_pred], true_cols [m][k] and certified [m] of the same m')
    total, rows = 0.0, 0
    for p, t, c in zip(pred, true, cert):
        want = set(int(x) for x in t if x >= 0)
        if not c or not want:
            continue
        total += len(want & set(int(x) for x in p if x >= 0)) / len(want)
        rows += 1
    return (total / rows if rows else float('nan')), rows


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def _is_csr(store):
    from .web import CsrStore
    return isinstance(store, CsrStore)


def _csr_ged_grid(store, q_idx, db_idx, both_orders, bounds, mapping, device, ld, return_status):
    import torch
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    struct = store.to_device(dev)
    G = len(store)
    q, db = _index(q_idx, dev), _index(db_idx, dev)
    m = G if q is None else int(q.numel())
    n = G if db is None else int(db.numel())
    ld = n if ld is None else int(ld)
    if ld < n:
        raise ValueError('ld {} below n {}'.format(ld, n))
    nbytes = _lib.csr_ged_grid_workspace_bytes(m, n, store.n_max)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=dev)
    ub = torch.empty((m, ld), dtype=torch.int32, device=dev)
    lb = torch.empty((m, ld), dtype=torch.int32, device=dev) if bounds else None
    mp = torch.empty((m, n, store.n_max), dtype=torch.int16, device=dev) if mapping else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.csr_ged_grid(struct, q, m, db, n, both_orders, ub, ld, lb, mp, status, ws)
    if not return_status:
        rc = int(status.item())
        if rc != 0:
            raise _lib.SiameseHipError('sg_csr_ged_grid: {} (a graph id outside the store, or a '
                                       'node count outside [1, n_max])'.format(
                                           _lib._ERR_NAMES.get(rc, rc)))
    out = [ub[:, :n]]
    if bounds:
        out.append(lb[:, :n])
    if mapping:
        out.append(mp)
    if return_status:
        out.append(status)
    return out[0] if len(out) == 1 else tuple(out)


class _ConstantEncoder(object):
    """Graphs without the node feature: one type."""

    def encode_columns(self, g):
        return [0] * g.number_of_nodes()

    def input_dim(self):
        return 1


def _type_encoder(graphs, node_feat_name):
    from .graphs import NodeFeatureOneHotEncoder
    if not graphs:
        raise ValueError('no graphs')
    have = [len(_attr(g, node_feat_name)) for g in graphs]
    if all(h == g.number_of_nodes() for h, g in zip(have, graphs)):
        enc = NodeFeatureOneHotEncoder(graphs, node_feat_name).pin_sorted()
    elif not any(have):
        enc = _ConstantEncoder()
    else:
        raise ValueError('some nodes have no {!r} attribute'.format(node_feat_name))
    return enc


def csr_store_of_graphs(graphs, node_feat_name='type'):
    """A web.CsrStore of networkx graphs for the GED calls, for graphs of at most 512 nodes:
    types are encoded as store_of_graphs encodes them."""
    from .graphs import ModelGraph
    from .web import CsrStore
    graphs = list(graphs)
    enc = _type_encoder(graphs, node_feat_name)
    nm = max(g.number_of_nodes() for g in graphs)
    if nm > GED_CSR_MAX_NODES:
        raise _lib.SiameseHipError('the bipartite GED bounds serve graph-store graphs of at most '
                                   '{} nodes (largest here: {})'.format(GED_CSR_MAX_NODES, nm))
    return CsrStore([ModelGraph(g, enc) for g in graphs], enc.input_dim())


def store_of_graphs(graphs, node_feat_name='type', n_max=None):
    """A GraphStore of networkx graphs for the GED calls: types are the graphs' node_feat_name
    values in sorted order (only their equality matters), n_max the largest node count unless
    given."""
    from .graphs import ModelGraph
    from .packer import GraphStore
    graphs = list(graphs)
    enc = _type_encoder(graphs, node_feat_name)
    nm = max(g.number_of_nodes() for g in graphs)
    n_max = max(nm, 1) if n_max is None else int(n_max)
    if n_max > GED_MAX_NODES:
        raise _lib.SiameseHipError('the bipartite GED bounds serve graphs of at most {} nodes '
                                   '(largest here: {})'.format(GED_MAX_NODES, nm))
    return GraphStore([ModelGraph(g, enc) for g in graphs], n_max, enc.input_dim())


def _largest(graphs):
    return max((g.number_of_nodes() for g in graphs), default=0)


def _attr(g, name):
    import networkx as nx
    return nx.get_node_attributes(g, name)


def ged_matrix(graphs_or_store, both_orders=True, device='cuda', node_feat_name='type',
               exact_budget=None, beam_width=None, refine_moves=None):
    """All-pairs upper bounds as a host int64 matrix [G][G], ready for
    DistCalculator.from_matrix.  With both_orders it is symmetric with a zero diagonal.
    With exact_budget=B: (matrix, proven), the budgeted search's ub and the bool matrix of the
    pairs whose distance it proved (ub is the exact distance there); with beam_width=w the
    same pair from the beam search, with refine_moves=k from the 2-exchange refinement (proven
    there: the refined ub meets the bipartite lb)."""
    store = graphs_or_store
    if not hasattr(store, 'to_device'):
        graphs = list(graphs_or_store)
        # the graph-store route has the bounds only: with exact_budget, beam_width or
        # refine_moves a graph of more than 32 nodes is refused by store_of_graphs, as before
        if _largest(graphs) > GED_MAX_NODES and exact_budget is None and beam_width is None \
                and refine_moves is None:
            store = csr_store_of_graphs(graphs, node_feat_name)
        else:
            store = store_of_graphs(graphs, node_feat_name)
    if exact_budget is not None or beam_width is not None or refine_moves is not None:
        ub, lb = ged_grid(store, both_orders=both_orders, bounds=True, device=device,
                          exact_budget=exact_budget, beam_width=beam_width,
                          refine_moves=refine_moves)
        ub, lb = ub.cpu().numpy().astype(np.int64), lb.cpu().numpy().astype(np.int64)
        return ub, ub == lb
    ub = ged_grid(store, both_orders=both_orders, device=device)
    return ub.cpu().numpy().astype(np.int64)


def ged_pair(g1, g2, device='cuda', node_feat_name='type', exact_budget=None, beam_width=None,
             refine_moves=None):
    """(ub, lb) of two networkx graphs through a two-graph store, ub the min over both
    assignment orders; with exact_budget=B those of the budgeted search (ub == lb: proven),
    with beam_width=w those of the beam search, with refine_moves=k those of the 2-exchange
    refinement."""
    # the graph-store route has the bounds only (with exact_budget, beam_width or refine_moves a
    # graph of more than 32 nodes is refused by store_of_graphs, as before)
    if _largest([g1, g2]) > GED_MAX_NODES and exact_budget is None and beam_width is None \
            and refine_moves is None:
        store = csr_store_of_graphs([g1, g2], node_feat_name)
    else:
        store = store_of_graphs([g1, g2], node_feat_name)
    ub, lb = ged_grid(store, [0], [1], both_orders=True, bounds=True, device=device,
                      exact_budget=exact_budget, beam_width=beam_width,
                      refine_moves=refine_moves)
    return int(ub.item()), int(lb.item())


def exact_label_matrix(graphs_or_store, device='cuda', node_feat_name='type',
                       budget=GED_EXACT_DEFAULT_BUDGET):
    """The label matrix of ged='exact' / ged_labels='exact': the budgeted search's ub for all
    pairs, with the number of pairs left unproven logged (their ub is the best path found, as
    the reference's AIDS10k labels are a minimum over approximate solvers)."""
    import logging
    dmat, proven = ged_matrix(graphs_or_store, device=device, node_feat_name=node_feat_name,
                              exact_budget=budget)
    logging.getLogger(__name__).info(
        'exact GED labels: %d of %d pairs left unproven within %d expansions',
        int((~proven).sum()), proven.size, budget)
    return dmat


def beam_label_matrix(graphs_or_store, width=GED_BEAM_DEFAULT_WIDTH, device='cuda',
                      node_feat_name='type'):
    """The label matrix of ged='lbeam<w>' / ged_labels='lbeam<w>': the beam search's ub for all
    pairs, with the number of pairs left unproven logged (their ub is the best path found)."""
    import logging
    dmat, proven = ged_matrix(graphs_or_store, device=device, node_feat_name=node_feat_name,
                              beam_width=width)
    logging.getLogger(__name__).info(
        'beam GED labels: %d of %d pairs left unproven at width %d',
        int((~proven).sum()), proven.size, width)
    return dmat


def refine_label_matrix(graphs_or_store, moves=GED_REFINE_DEFAULT_MOVES, device='cuda',
                        node_feat_name='type'):
    """The label matrix of ged='bpswap' / ged_labels='bpswap': the refined bipartite ub for all
    pairs, with the number of pairs left unproven logged (their ub is the best path found)."""
    import logging
    dmat, proven = ged_matrix(graphs_or_store, device=device, node_feat_name=node_feat_name,
                              refine_moves=moves)
    logging.getLogger(__name__).info(
        'refined GED labels: %d of %d pairs left unproven within %d moves per start',
        int((~proven).sum()), proven.size, moves)
    return dmat


def beam_width_of(name):
    """The width w of an algorithm / label name 'lbeam<w>' (w in [1, 128]), or None for any
    other name; a width outside the range raises."""
    import re
    mt = re.fullmatch(r'lbeam(\d+)', name) if isinstance(name, str) else None
    if mt is None:
        return None
    w = int(mt.group(1))
    if not 1 <= w <= _lib.GED_BEAM_MAX_WIDTH:
        raise RuntimeError('{!r}: the beam width is in [1, {}]'.format(
            name, _lib.GED_BEAM_MAX_WIDTH))
    return w
