"""Graph distances (src/distance.py).

Only `normalized_dist` (distance.py:59-60) is on the hot path.  `ged` and `mcs`
shell out to the Java graph-matching-toolkit / the `chorus` library in the
reference (distance.py:10-56); those solvers are out of scope here and raise
unless a cached distance exists (see dist_calculator.DistCalculator).  The one
algorithm computed here is 'bp', the bipartite upper bound on the device
(graphembedding_amd.ged, include/siamese_ged.h).
"""
from __future__ import annotations


def normalized_dist(d, g1, g2):
    return 2 * d / (g1.number_of_nodes() + g2.number_of_nodes())


def ged(g1, g2, algo, debug=False, timeit=False):
    """algo='bp': the bipartite (Riesen & Bunke) upper bound under the toolkit's AIDS cost
    model, the smaller of both assignment orders (the reference's `_revtakemin` caches), for
    graphs of at most 32 nodes.  The name is deliberately not 'hungarian': that the toolkit's
    Hungarian mode builds the same cost matrix (node costs plus local degree differences) and
    breaks ties the same way has not been checked, so its values are not claimed.  Every
    other algo raises: exact A* and beam search are out of scope."""
    if algo == 'bp':
        from .ged import ged_pair
        return ged_pair(g1, g2)[0]
    raise RuntimeError(
        'GED ground truth needs the external Java graph-matching-toolkit '
        '(reference src/distance.py:23-56); it is out of scope of this build. '
        'Provide a cached gid-pair distance map instead.')


def mcs(g1, g2):
    raise RuntimeError('MCS needs the external chorus library (reference src/distance.py:10-20).')
