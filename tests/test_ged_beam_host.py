"""The yardstick of the beam-search GED (tests/_ged_beam_restatement.py) against an independent
solver and against its own contract, on the host: lb <= GED <= ub <= the bipartite ub at every
width, lb == ub only at the exact distance, the map induces ub, width 0 is the seed, and a width
that cuts no level equals the unlimited exact search.  Then what test_gpu_ged_beam.py relies
on: which pairs of its grids are truncated, proven, pruned empty or seeded by the 2->1 order.

Nothing here asserts that ub falls as the width grows: a level-synchronous beam is not monotone.
"""
import numpy as np
import pytest

import _ged_beam_cases as BC
import _ged_beam_restatement as B
import _ged_exact_restatement as X
import _ged_restatement as R
from test_ged_exact_host import _exact, _random_connected

HOST_WIDTHS = (1, 2, 7, 128)


@pytest.fixture(scope='module')
def graphs():
    """test_ged_exact_host.py's 17 small graphs (the same seed and recipe)."""
    rng = np.random.default_rng(20)
    gs = [_random_connected(rng, n) for n in (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 5)]
    return gs + [_random_connected(rng, 6, p_extra=p) for p in (0.1, 0.3, 0.5)]


@pytest.fixture(scope='module')
def pairs(graphs):
    """{(i, j): (GED by networkx, seed)} for i <= j and for the pairs with a 6-node side in
    both orders, as test_ged_exact_host.py solves them."""
    G = len(graphs)
    out = {}
    for i in range(G):
        for j in range(G):
            if i <= j or max(i, j) >= G - 3:
                out[(i, j)] = (_exact(graphs[i], graphs[j]), X.seed(graphs[i], graphs[j]))
    return out


def test_bounds_hold_at_every_width(graphs, pairs):
    n_cut = n_proven_by_search = 0
    for (i, j), (ged, seeded) in pairs.items():
        g1, g2 = graphs[i], graphs[j]
        for w in HOST_WIDTHS:
            ub, lb, phi, e = B.beam_pair(g1, g2, w, seeded)
            assert lb <= ged <= ub <= seeded[0], (i, j, w)
            assert lb != ub or ub == ged, (i, j, w)
            assert R.induced_cost(g1, g2, phi) == ub, (i, j, w)
            kept = [x for x in phi if x >= 0]
            assert len(phi) == len(g1[0]) and len(set(kept)) == len(kept)
            assert all(x < len(g2[0]) for x in kept)
            assert 0 <= e <= 1 + (len(g1[0]) - 1) * w
            cut = B.is_truncated(g1, g2, w, seeded)
            assert lb == (seeded[1] if cut else ub)
            n_cut += cut
            n_proven_by_search += e > 0 and not cut
    assert n_cut > 0 and n_proven_by_search > 0


def test_width_zero_is_the_seed(graphs):
    for g1 in graphs:
        for g2 in graphs:
            ub, lb, phi, e = B.beam_pair(g1, g2, 0)
            wub, wlb, _ = R.bp_pair(g1, g2, both_orders=True)
            assert (ub, lb, e) == (wub, wlb, 0) and phi == X.seed(g1, g2)[2]


def test_a_width_that_cuts_no_level_is_the_exact_search(graphs, pairs):
    """The largest level of the unlimited beam gives the width from which on nothing is cut:
    there the beam equals the unlimited depth-first restatement's distance, is proven, and
    expands what the unlimited beam expands; one below that width a level is cut."""
    n_below = 0
    for (i, j), (ged, seeded) in pairs.items():
        g1, g2 = graphs[i], graphs[j]
        if not B.searched(seeded[0], seeded[1], None):
            continue
        _, e_all, leaf, survivors = B.search(g1, g2, seeded[0], None)
        w = max(survivors[:-1] + [1])       # the last level's survivors are leaves: never cut
        ub, lb, phi, e = B.beam_pair(g1, g2, w, seeded)
        assert not B.is_truncated(g1, g2, w, seeded)
        assert ub == lb == X.exact_pair(g1, g2, None)[0] == ged and e == e_all, (i, j)
        if w > 1:
            assert B.is_truncated(g1, g2, w - 1, seeded), (i, j)
            n_below += 1
    assert n_below > 0


@pytest.fixture(scope='module')
def gpu_plan():
    """[(set, width, a, b, (ub, lb, phi, expanded), truncated)] over the GPU test's grids."""
    out = []
    for name, widths, q, db in BC.GRIDS:
        _, ref = BC.store(name)
        for w in widths:
            for a in BC.ids(name, q):
                for b in BC.ids(name, db):
                    res, cut = ref.run(a, b, w)
                    out.append((name, w, a, b, res, cut))
    return out


def test_gpu_grids_reach_both_branches_of_the_lb_rule_at_every_width(gpu_plan):
    """At every width the GPU test runs, some pair is truncated (lb stays the seed's) and some
    pair is searched to the end (lb = ub); width 0 searches nothing."""
    assert {w for _, w, _, _, _, _ in gpu_plan} == set(BC.WIDTHS)
    n32 = [g.number_of_nodes() for g in BC.graphs('b32')]
    for w in BC.WIDTHS:
        rows = [r for r in gpu_plan if r[1] == w]
        cut = [r for r in rows if r[5]]
        whole = [r for r in rows if r[4][3] > 0 and not r[5]]
        print('width {}: {} pairs, {} truncated, {} searched to the end'.format(
            w, len(rows), len(cut), len(whole)))
        if w == 0:
            assert not cut and not whole and any(r[4][0] != r[4][1] for r in rows)
            continue
        assert cut and whole, w
        assert all(r[4][1] == r[4][0] for r in whole)
        assert any(r[4][1] < r[4][0] for r in cut), w
        assert {r[0] for r in cut} == {r[0] for r in rows}, w    # in every set run at w
        if w in (65, 128):           # 32 levels without a cut: the pair built for it
            assert any(r[0] == 'b32' and n32[r[2]] == 32 and r[4][3] > 32 for r in whole), w


def test_gpu_grids_hold_the_cases_the_kernel_can_get_wrong(gpu_plan):
    for name in ('b10', 'b32'):
        _, ref = BC.store(name)
        n = [g.number_of_nodes() for g in BC.graphs(name)]
        rows = [r for r in gpu_plan if r[0] == name]
        # a pair seeded by the inverse of the 2->1 assignment
        assert any(R.upper_bound(ref.graph(b), ref.graph(a))[0] <
                   R.upper_bound(ref.graph(a), ref.graph(b))[0]
                   for a in range(len(n)) for b in range(len(n))), name
        # a level with fewer survivors than the width, and a beam that pruning empties
        few = empty = better = 0
        for _, w, a, b, res, cut in rows:
            survivors = ref.survivors.get((a, b, w))
            if survivors is None:         # not searched, or the run of a smaller width
                continue
            few += any(0 < x < w for x in survivors[:-1])
            empty += survivors[-1] == 0
            better += res[0] < ref.seed(a, b)[0]
        assert few and empty and better, (name, few, empty, better)
    # 33 children and 32 levels: both orders of the 31- and 32-node graphs, searched
    big = [r for r in gpu_plan if r[0] == 'b32' and r[4][3] > 0]
    n = [g.number_of_nodes() for g in BC.graphs('b32')]
    assert any(n[r[2]] == 32 and n[r[3]] == 31 for r in big)
    assert any(n[r[2]] == 31 and n[r[3]] == 32 for r in big)
    assert any(n[r[2]] == 32 and n[r[3]] == 32 and r[1] == 128 and r[5] for r in big)
    assert max(r[4][3] for r in big) > 1 + 30 * 128
