"""The restatement of include/siamese_ged_refine.h (tests/_ged_refine_restatement.py) against
checks that do not share its code: the induced cost of every accepted move's map, the bipartite
bounds, the exact search's proven distances; then what the budgets do, that every kind of move is
accepted, the figures of the full b10 set, and that the shared cases (_ged_refine_cases.py) hold
what test_gpu_ged_refine.py relies on.  No GPU."""
import numpy as np
import pytest

import _ged_exact_restatement as X
import _ged_refine_cases as RC
import _ged_refine_restatement as F
import _ged_restatement as R

SETS = ('b10', 'b32', 'r32')
EXACT_BUDGET = 3000      # expansions of the exact restatement per b10 pair


def _pairs(name):
    G = len(RC.graphs(name))
    return [(a, b) for a in range(G) for b in range(G)]


@pytest.mark.parametrize('name', SETS)
def test_every_accepted_move_costs_what_induced_cost_says(name):
    """The incremental cost of each accepted move is the full induced cost of its map, the map
    stays injective, and each move lowers the cost."""
    _, ref = RC.store(name)
    moved = 0
    for a, b in _pairs(name):
        g1, g2 = ref.graph(a), ref.graph(b)
        s = ref.seed(a, b)
        for k, path in enumerate(ref.descents(a, b)):
            cost, phi = s[k]
            assert R.induced_cost(g1, g2, phi) == cost, (a, b, k)
            for c, p, ma, mx, kind in path:
                kept = [x for x in p if x >= 0]
                assert len(set(kept)) == len(kept) and len(p) == len(g1[0]) and p[ma] == mx
                assert all(-1 <= x < len(g2[0]) for x in p)
                assert R.induced_cost(g1, g2, p) == c < cost, (a, b, k)
                assert sum(x != y for x, y in zip(p, phi)) <= 2 and kind in F.KINDS
                cost, phi = c, p
                moved += 1
            assert len(path) <= s[k][0] - s[2]          # the counted loop's ceiling
    assert moved > 100


@pytest.mark.parametrize('name', SETS)
def test_bounds_hold_at_every_budget(name):
    _, ref = RC.store(name)
    for budget in RC.BUDGETS[name]:
        for a, b in _pairs(name):
            s = ref.seed(a, b)
            bp = min(s[0][0], s[1][0])
            ub, lb, phi, moves = ref.pair(a, b, budget)
            assert lb == s[2] <= ub <= bp, (a, b, budget)
            assert R.induced_cost(ref.graph(a), ref.graph(b), phi) == ub, (a, b, budget)
            assert 0 <= moves <= 2 * budget and moves <= (s[0][0] - lb) + (s[1][0] - lb)
            assert moves > 0 or ub == bp


def test_refined_ub_is_never_below_a_proven_distance():
    _, ref = RC.store('b10')
    proven = below = 0
    for a, b in _pairs('b10'):
        xub, xlb, _, _ = X.exact_pair(ref.graph(a), ref.graph(b), EXACT_BUDGET)
        ub = ref.pair(a, b, F.MAX_MOVES)[0]
        if xub == xlb:
            proven += 1
            assert ub >= xub, (a, b)
            below += ub > xub
        else:
            assert ub >= xlb
    assert proven > 100 and below > 0        # the descent stops at local optima


@pytest.mark.parametrize('name', SETS)
def test_budget_zero_is_the_seed_and_the_full_budget_is_m(name):
    _, ref = RC.store(name)
    most, differs = 0, 0
    for a, b in _pairs(name):
        g1, g2 = ref.graph(a), ref.graph(b)
        want = X.seed(g1, g2)
        ub, lb, phi, moves = ref.pair(a, b, 0)
        assert (ub, lb, phi, moves) == (want[0], want[1], want[2], 0), (a, b)
        most = max([most] + [len(p) for p in ref.descents(a, b)])
        s = ref.seed(a, b)
        if s[2] == min(s[0][0], s[1][0]):                # skipped at every budget
            assert ref.pair(a, b, F.MAX_MOVES) == ref.pair(a, b, 0)
    M = RC.MOST[name]
    assert most == M and RC.BUDGETS[name] == tuple(sorted({0, 1, M - 1, M, F.MAX_MOVES}))
    for a, b in _pairs(name):
        assert ref.pair(a, b, M) == ref.pair(a, b, F.MAX_MOVES)
        differs += ref.pair(a, b, M - 1) != ref.pair(a, b, M)
        one = ref.pair(a, b, 1)
        assert one[3] <= 2 and one[0] <= ref.pair(a, b, 0)[0]
    assert differs >= 1


def test_pair_and_grid_agree_with_the_uncached_functions():
    s, ref = RC.store('r32')
    for a, b in RC.ROUNDS.values():
        for budget in (0, 1, 2, F.MAX_MOVES):
            assert F.refine_pair(ref.graph(a), ref.graph(b), budget) == ref.pair(a, b, budget)
    ub, lb, mp, mv = ref.grid([1, -1, 3], [2, 4, 99], 2)
    assert (ub[1] == -1).all() and (mv[:, 2] == -1).all() and (mp[1] == -1).all()
    assert (ub[0, 0], lb[0, 0], mv[0, 0]) == ref.pair(1, 2, 2)[:2] + (ref.pair(1, 2, 2)[3],)
    assert list(mp[0, 0, :7]) == ref.pair(1, 2, 2)[2] and (mp[0, 0, 7:] == -1).all()


def test_every_kind_of_move_is_accepted():
    """Exchange, move onto a free node and hand-over occur in the cases' descents.  Both
    bipartite maps leave min(n1, n2) nodes mapped and none of those three changes that number,
    so no descent from a seed un-deletes; that kind is shown from a constructed map, through the
    same descend()."""
    seen = set()
    for name in SETS:
        _, ref = RC.store(name)
        for a, b in _pairs(name):
            s = ref.seed(a, b)
            for k, path in enumerate(ref.descents(a, b)):
                assert sum(x >= 0 for x in s[k][1]) == min(len(s[k][1]), len(ref.graph(b)[0]))
                seen |= {step[4] for step in path}
    assert seen == {'exchange', 'free', 'handover'}
    # a path a-b-c against itself, from the map that deletes b and leaves its image free
    t = np.zeros(3, dtype=np.int64)
    A = np.zeros((3, 3), dtype=bool)
    A[0, 1] = A[1, 0] = A[1, 2] = A[2, 1] = True
    g = (t, A)
    start = [0, -1, 2]
    cost = R.induced_cost(g, g, start)
    assert cost == 6
    path = F.descend(g, g, start, cost)
    assert [(c, p, k) for c, p, _, _, k in path] == [(0, [0, 1, 2], 'undelete')]
    # and a deleted node next to a mapped one whose image suits it better: a hand-over
    assert F.kind_of(-1, 2) == 'handover' and F.kind_of(1, -1) == 'free'
    assert F.kind_of(1, 2) == 'exchange' and F.kind_of(-1, -1) == 'undelete'


def test_the_best_move_is_the_smallest_cost_then_a_then_x():
    """The one-type complete graph on 4 nodes against itself, from a map that deletes nodes 2
    and 3: four un-deletions tie on cost, and the smallest (a, x) is taken."""
    t = np.zeros(4, dtype=np.int64)
    A = ~np.eye(4, dtype=bool)
    g = (t, A)                                  # the complete graph on 4 nodes, one type
    start = [1, 0, -1, -1]
    path = F.descend(g, g, start, R.induced_cost(g, g, start))
    # every un-deletion of node 2 or 3 onto node 2 or 3 lowers the cost alike: (2, 2) is first
    assert [(a, x) for _, _, a, x, _ in path] == [(2, 2), (3, 3)]
    assert path[-1][0] == 0


def test_the_prototype_figures_on_the_full_b10_set():
    _, ref = RC.store('b10')
    lowered = slack0 = slack1 = met0 = met1 = most = 0
    for a, b in _pairs('b10'):
        s = ref.seed(a, b)
        bp = min(s[0][0], s[1][0])
        ub, lb, _, moves = ref.pair(a, b, F.MAX_MOVES)
        lowered += ub < bp
        slack0, slack1 = slack0 + bp - lb, slack1 + ub - lb
        met0, met1 = met0 + (bp == lb), met1 + (ub == lb)
        most = max(most, moves)
    assert len(_pairs('b10')) == 169 and lowered == 71
    assert (slack0, slack1) == (536, 208) and (met0, met1) == (85, 101) and most == 7


def test_the_cases_hold_the_rounds_the_kernel_can_get_wrong():
    s, ref = RC.store('r32')
    assert sorted(RC.ROUNDS) == [1, 63, 64, 65, 1024]
    for k, (a, b) in RC.ROUNDS.items():
        assert int(s.n[a]) * int(s.n[b]) == k
        assert (ref.pair(a, b, F.MAX_MOVES)[3] > 0) == (k > 1), k
    assert (int(s.n[1]), int(s.n[2])) == (7, 9) and (int(s.n[5]), int(s.n[6])) == (5, 13)
    # b32 keeps its 32 x 32 pairs in both orders, refined ones among them, and pairs where
    # start 1 wins, where start 0 wins after a tie of the seeds, and with n1 > n2 and n1 < n2
    s32, r32 = RC.store('b32')
    big = [g for g in range(len(s32.n)) if int(s32.n[g]) == 32]
    assert len(big) >= 4
    assert all(r32.pair(a, b, F.MAX_MOVES)[3] > 0 for a in big[:2] for b in big[:2] if a != b)
    first = second = 0
    for name in SETS:
        _, ref = RC.store(name)
        for a, b in _pairs(name):
            sd = ref.seed(a, b)
            c0 = F.at_budget(sd[0], ref.descents(a, b)[0], F.MAX_MOVES)[0]
            c1 = F.at_budget(sd[1], ref.descents(a, b)[1], F.MAX_MOVES)[0]
            if ref.descents(a, b)[0]:
                first += c0 <= c1 and sd[1][0] < sd[0][0]     # the seed's choice turned round
                second += c1 < c0 and sd[0][0] <= sd[1][0]
    assert first > 0 and second > 0
