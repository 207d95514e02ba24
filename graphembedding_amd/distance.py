"""Graph distances (src/distance.py).

Only `normalized_dist` (distance.py:59-60) is on the hot path.  `ged` and `mcs`
shell out to the Java graph-matching-toolkit / the `chorus` library in the
reference (distance.py:10-56); those solvers are out of scope here and raise
unless a cached distance exists (see dist_calculator.DistCalculator).  Four
algorithms are computed here, on the device (graphembedding_amd.ged): 'bp', the
bipartite upper bound (include/siamese_ged.h; include/siamese_ged_csr.h for graphs
of 33 to 512 nodes), 'exact', the budgeted branch
and bound seeded with it (include/siamese_ged_exact.h), 'lbeam<w>', the
level-synchronous beam search seeded with it (include/siamese_ged_beam.h), and
'bpswap', the 2-exchange refinement of its maps (include/siamese_ged_refine.h).
`mcs` is computed on the device too (graphembedding_amd.mcs, include/siamese_mcs.h):
the maximum common induced subgraph under type equality, which is not chorus's
MCS-DR.
"""
from __future__ import annotations


def normalized_dist(d, g1, g2):
    return 2 * d / (g1.number_of_nodes() + g2.number_of_nodes())


def ged(g1, g2, algo, debug=False, timeit=False):
    """algo='bp': the bipartite (Riesen & Bunke) upper bound under the toolkit's AIDS cost
    model, the smaller of both assignment orders (the reference's `_revtakemin` caches), for
    graphs of at most 512 nodes (above 32 nodes through the graph-store call of
    include/siamese_ged_csr.h, same construction and tie rules).  The name is deliberately
    not 'hungarian': that the toolkit's Hungarian mode builds the same cost matrix (node costs
    plus local degree differences) and breaks ties the same way has not been checked, so its
    values are not claimed.

    algo='exact': the exact distance under the same cost model, proven by the budgeted branch
    and bound within ged.GED_EXACT_DEFAULT_BUDGET = 2^20 expansions; a pair it cannot prove
    (more than 16 nodes, or the budget spent) raises with the bounds it has.  The name is not
    'astar': the value is the same distance, the program is not the toolkit's.

    algo='lbeam<w>' (w in [1, 128], e.g. 'lbeam80'): the upper bound of the level-synchronous
    beam search of width w (include/siamese_ged_beam.h), seeded with 'bp' and never above it,
    for graphs of at most 32 nodes; a width outside [1, 128] raises.  The name is not
    'beam<w>': the toolkit's beam search is best-first over a truncated OPEN list, this one
    keeps the w best states of every level, so its values are not claimed to be the toolkit's.

    algo='bpswap': 'bp' after local search on the node map (include/siamese_ged_refine.h): the
    2-exchange refinement of both assignment orders' maps within ged.GED_REFINE_DEFAULT_MOVES
    = 1024 accepted moves per start, never above 'bp', for graphs of at most 32 nodes.  The
    name is this project's; no toolkit value is claimed.

    Every other algo raises: the toolkit's own A*, beam search ('beam80'), 'hungarian' and 'vj'
    are out of scope."""
    if algo == 'bp':
        from .ged import ged_pair
        return ged_pair(g1, g2)[0]
    if algo == 'bpswap':
        from .ged import GED_REFINE_DEFAULT_MOVES, ged_pair
        return ged_pair(g1, g2, refine_moves=GED_REFINE_DEFAULT_MOVES)[0]
    if isinstance(algo, str) and algo.startswith('lbeam'):
        from .ged import beam_width_of, ged_pair
        w = beam_width_of(algo)
        if w is not None:
            return ged_pair(g1, g2, beam_width=w)[0]
    if algo == 'exact':
        from .ged import GED_EXACT_DEFAULT_BUDGET, ged_pair
        ub, lb = ged_pair(g1, g2, exact_budget=GED_EXACT_DEFAULT_BUDGET)
        if ub != lb:
            raise RuntimeError('exact GED not proven within {} expansions: ub {} lb {}'.format(
                GED_EXACT_DEFAULT_BUDGET, ub, lb))
        return ub
    raise RuntimeError(
        'GED ground truth needs the external Java graph-matching-toolkit '
        '(reference src/distance.py:23-56); it is out of scope of this build. '
        'Provide a cached gid-pair distance map instead.')


def mcs(g1, g2, connected=False):
    """The node count of a maximum common induced subgraph of g1 and g2 under type equality
    (with connected=True of a connected one), proven by the budgeted McSplit search of
    include/siamese_mcs.h within mcs.MCS_DEFAULT_BUDGET = 2^20 expansions; a pair it cannot
    prove raises with the size and the bound it has.  Graphs of at most 32 nodes.

    It is not chorus's MCS-DR bond count (reference src/distance.py:10-20: a connected maximum
    common edge subgraph over atom and bond labels): chorus's values are not claimed."""
    from . import mcs as _mcs
    size, bound, _ = _mcs.mcs_pair(g1, g2, connected=connected, budget=_mcs.MCS_DEFAULT_BUDGET)
    if size != bound:
        raise RuntimeError('MCS not proven within {} expansions: size {} bound {}'.format(
            _mcs.MCS_DEFAULT_BUDGET, size, bound))
    return size
