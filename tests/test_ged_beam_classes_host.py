"""What test_gpu_ged_beam_classes.py relies on, derived on the host from the beam restatement
(tests/_ged_beam_restatement.py) over the sets of _ged_beam_classes.py: which pairs of every
grid are truncated and which are searched to the end, that the dense set drives the packed state
word, the all-tie selection and the 32-bit masks to their limits (by a tracing copy of the
restatement's loop, checked against it), that the restatement obeys the closed forms, and that
the large grid really takes two grid rows.

Measured: the whole file takes 34 s on one CPU core: 24 s for the restatement over every grid
(half of it the dense set at widths 64, 65 and 128) and 10 s for the tracing copy.
"""
from collections import Counter

import numpy as np
import pytest

import _ged_beam_cases as BC
import _ged_beam_classes as BK
import _ged_beam_restatement as B
import _ged_classes as K
import _ged_exact_restatement as X
import _ged_restatement as R

# what a class cannot provide, as (set, width, 'cut' | 'whole'): a pair truncated at the width,
# or a pair searched to the end.  Everything not listed here is asserted to be present.
#   dense32   the width never stops cutting: 31 levels of up to 33 tied children per state
#   edge0, planted9, cap1   the seed proves every pair (lb == ub), so nothing is searched
#   types29, planted16, cap7   the small widths cut every searched pair
NEVER_SEARCHED = BK.NEVER_SEARCHED
ABSENT = ({('dense32', w, 'whole') for w in BK.DENSE32_WIDTHS} |
          {(name, w, what) for name in NEVER_SEARCHED for w in BK.CLASS_WIDTHS
           for what in ('cut', 'whole')} |
          {(name, w, 'whole') for name in ('types29', 'planted16') for w in (1, 7)} |
          {('cap7', 1, 'whole')})
SEARCHED = tuple(name for name in BK.SETS if name not in NEVER_SEARCHED)
assert set(SEARCHED) == {'forest', 'types29', 'planted16', 'dense32', 'cap7'}


@pytest.fixture(scope='module')
def plan():
    """{(set, width): {(a, b): ((ub, lb, phi, expanded), truncated)}} over the GPU test's grids."""
    out = {}
    for name, widths in BK.GRIDS:
        _, ref = BK.store(name)
        G = len(BK.graphs(name))
        for w in widths:
            out[(name, w)] = {(a, b): ref.run(a, b, w) for a in range(G) for b in range(G)}
    return out


def test_every_grid_has_a_truncated_pair_and_one_searched_to_the_end(plan):
    for (name, w), rows in plan.items():
        cut = [k for k, (res, c) in rows.items() if c]
        whole = [k for k, (res, c) in rows.items() if res[3] > 0 and not c]
        print('{} width {}: {} pairs, {} truncated, {} searched to the end'.format(
            name, w, len(rows), len(cut), len(whole)))
        assert bool(cut) == ((name, w, 'cut') not in ABSENT), (name, w, cut[:3])
        assert bool(whole) == ((name, w, 'whole') not in ABSENT), (name, w, whole[:3])
        assert all(res[1] == res[0] for res, c in rows.values() if res[3] > 0 and not c)
        assert all(res[1] == BK.store(name)[1].seed(a, b)[1]
                   for (a, b), (res, c) in rows.items() if c)
    assert set(SEARCHED) | set(NEVER_SEARCHED) == set(BK.SETS)
    for name in BK.SETS:
        for w in dict(BK.GRIDS)[name]:
            assert any(res[3] > 0 for res, _ in plan[(name, w)].values()) == (name in SEARCHED)
    # a pair with an edgeless side is never searched, in any set: every graph-2 node is
    # substituted or inserted, so its degree is paid once whatever the assignment, the
    # assignment problem minimises the type cost alone and lb == ub.  The search's E1 = 0
    # and E2 = 0 cases are therefore out of reach of any test
    for (name, w), rows in plan.items():
        gs = BK.graphs(name)
        for (a, b), (res, _) in rows.items():
            if 0 in (gs[a].number_of_edges(), gs[b].number_of_edges()):
                assert res[3] == 0 and res[0] == res[1], (name, w, a, b)
    # forests with an isolated node and the 29 types, searched
    gs = BK.graphs('forest')
    assert any(res[3] > 0 and min(dict(gs[a].degree()).values()) == 0
               for (a, b), (res, _) in plan[('forest', 128)].items())
    assert len({t for g in BK.graphs('types29') for _, t in g.nodes(data='type')}) >= 16


def test_dense32_pairs_the_seed_leaves_open(plan):
    """K_32 - pm against K_31, K_17, K_16 and K_9 and K_32 - e against K_31, in both orders
    (10 ordered pairs), are the pairs the seed leaves unproven (K_32 - e against K_17, K_16 and
    K_9 it proves).  Each is searched and truncated at every width, and the search improves on
    the seed except for K_32 - pm against K_31."""
    _, ref = BK.store('dense32')
    pairs = [(2, b) for b in (3, 4, 5, 6)] + [(1, 3)]
    pairs += [(b, a) for a, b in pairs]
    G = len(BK.DENSE32)
    assert sorted(pairs) == [(a, b) for a in range(G) for b in range(G)
                             if ref.seed(a, b)[1] < ref.seed(a, b)[0]]
    assert ref.seed(2, 6)[:2] == (475, 467) and ref.seed(2, 3)[:2] == (46, 16)
    assert ref.seed(2, 4)[:2] == (375, 359)
    for a, b in pairs:
        s = ref.seed(a, b)
        for w in BK.DENSE32_WIDTHS:
            res, cut = plan[('dense32', w)][(a, b)]
            assert cut and res[3] > 0 and res[1] == s[1], (a, b, w)
        best = min(plan[('dense32', w)][(a, b)][0][0] for w in BK.DENSE32_WIDTHS)
        assert (best < s[0]) == ({a, b} != {2, 3}), (a, b, best, s[0])
    assert plan[('dense32', 128)][(2, 6)][0][0] == 467
    assert plan[('dense32', 128)][(2, 4)][0][0] == 361


def _trace(g1, g2, incumbent, width):
    """_ged_beam_restatement.search with a record of what the kernel's state word, selection and
    masks hold: (truncated, expanded, leaf, survivors) as search returns them, and the largest
    EU (graph-2 edges between used nodes) and g of a state kept for the next level, the largest
    number of unpruned children of one level that share one f, and whether a kept state has
    bit 31 of `used` set."""
    P = X._Pair(g1, g2)
    n1, n2 = P.n1, P.n2
    hmemo = {}

    def h(k, used):
        if (k, used) not in hmemo:
            hmemo[(k, used)] = P.h(k, used)
        return hmemo[(k, used)]

    def eu(used):
        return sum(bin(P.m2[j] & used).count('1') for j in range(n2) if (used >> j) & 1) // 2

    seen = dict(EU=0, g=0, ties=0, bit31=False, I=0)
    level = [(0, 0, [])]
    expanded, truncated, survivors = 0, False, []
    for k in range(n1):
        children = []
        for p, (g, used, phi) in enumerate(level):
            expanded += 1
            for c in [j for j in range(n2) if not (used >> j) & 1] + [n2]:
                gc = g + P.step(phi, c)
                uc = used | (1 << c) if c < n2 else used
                f = gc + h(k + 1, uc)
                if f < incumbent:
                    children.append((f, p, c, gc, uc))
        survivors.append(len(children))
        children.sort()
        if not children:
            return (truncated, expanded, None, survivors), seen
        seen['ties'] = max(seen['ties'], max(Counter(c[0] for c in children).values()))
        if k == n1 - 1:
            f, p, c = children[0][:3]
            leaf = (f, level[p][2] + [c if c < n2 else -1])
            return (truncated, expanded, leaf, survivors), seen
        if len(children) > width:
            truncated = True
            children = children[:width]
        level = [(gc, uc, level[p][2] + [c if c < n2 else -1]) for f, p, c, gc, uc in children]
        for gc, uc, _ in level:
            rem2 = [P.t2[j] for j in range(n2) if not (uc >> j) & 1]
            seen['EU'] = max(seen['EU'], eu(uc))
            seen['g'] = max(seen['g'], gc)
            seen['I'] = max(seen['I'], sum((Counter(P.t1[k + 1:]) & Counter(rem2)).values()))
            seen['bit31'] = seen['bit31'] or bool((uc >> 31) & 1)
    raise AssertionError('n1 >= 1 levels')


def test_dense32_reaches_the_limits_of_the_state_word_the_selection_and_the_masks(plan):
    """Over the searched pairs of dense32 at width 128: a kept state with EU >= 256 (bit 8 of
    the 10-bit field, next to I), one with g >= 256, a level with at least two wavefronts' worth
    (128) of candidates sharing one f, whose cut falls inside a 64-candidate chunk, and a kept
    state with bit 31 of `used` set.  The tracing copy returns what the restatement returns."""
    _, ref = BK.store('dense32')
    top = dict(EU=0, g=0, ties=0, bit31=False, I=0)
    for (a, b), (res, cut) in plan[('dense32', 128)].items():
        if res[3] == 0:
            continue
        s = ref.seed(a, b)
        got, seen = _trace(ref.graph(a), ref.graph(b), s[0], 128)
        assert got == B.search(ref.graph(a), ref.graph(b), s[0], 128), (a, b)
        for key in top:
            top[key] = max(top[key], seen[key])
    print('dense32 at width 128:', top)
    assert top['EU'] >= 256 and top['g'] >= 256 and top['ties'] >= 2 * 64 and top['bit31']
    assert top['EU'] < 1 << 10 and top['g'] < 1 << 16 and top['I'] == 31 < 1 << 6
    # widths 7 and 65 are no multiple of the 64 lanes: on K_9 against K_32 - pm (33 children a
    # state) the cut at `want` falls inside a chunk of a tie class of more than two chunks
    for w in (7, 65):
        s = ref.seed(6, 2)
        got, seen = _trace(ref.graph(6), ref.graph(2), s[0], w)
        assert got[0] and seen['ties'] >= 2 * 64 and plan[('dense32', w)][(6, 2)][1], w


@pytest.mark.parametrize('name', ['dense32', 'edge0'])
def test_the_restatement_obeys_the_closed_forms(plan, name):
    known = BK.closed_form(name)
    G = len(BK.graphs(name))
    assert len(known) == (G * G if name == 'edge0' else G * G - 2)   # all but K_32-e : K_32-pm
    n_proven = 0
    for w in dict(BK.GRIDS)[name]:
        for (a, b), value in known.items():
            ub, lb = plan[(name, w)][(a, b)][0][:2]
            assert lb <= value <= ub, (name, w, a, b)
            assert lb != ub or ub == value, (name, w, a, b)
            n_proven += lb == ub
    assert n_proven > 0
    if name == 'dense32':
        assert known[(2, 6)] == known[(6, 2)] == 467 and known[(2, 3)] == 46
        assert known[(0, 3)] == 1 + 31 and known[(1, 0)] == 1 and known[(0, 2)] == 16


def test_planted_copies_are_found_at_width_128(plan):
    """(g, pi(g)) of the planted sets: ub 0 and a map that is an isomorphism; the other pairs
    obey their planted bounds at every width."""
    for name in ('planted16', 'planted9'):
        gs = BK.graphs(name)
        for a, b in ((0, 1), (1, 0)):
            ub, lb, phi, _ = plan[(name, 128)][(a, b)][0]
            assert ub == lb == 0 and K.is_isomorphism(gs[a], gs[b], phi), (name, a, b)
        for w in BK.CLASS_WIDTHS:
            for (a, b), rule in K.known(name).items():
                ub, lb = plan[(name, w)][(a, b)][0][:2]
                assert lb <= rule[1] and (rule[0] == 'le' or lb != ub or ub == rule[1])


def test_capacity_sets():
    """The restored b10 stores hold the graphs of the capacity-10 store, so one restatement
    serves them all; cap1 and cap7 fill their capacities."""
    base, _ = BC.store('b10')
    G = len(base)
    assert max(base.n) == 10 and BK.RESTORED == (16, 17, 31, 32)
    for c in BK.RESTORED:
        s = BK.restored(c)
        assert s.n_max == c and np.array_equal(s.n, base.n)
        for g in range(G):
            (t, A), (wt, wA) = R.graph_of_store(s, g), R.graph_of_store(base, g)
            assert np.array_equal(t, wt) and np.array_equal(A, wA)
    s1, _ = BK.store('cap1')
    assert s1.n_max == 1 and s1.n.tolist() == [1] * 4 and len(set(s1.types[:, 0].tolist())) == 3
    s7, _ = BK.store('cap7')
    assert s7.n_max == 7 and sorted(set(s7.n.tolist())) == [1, 2, 3, 5, 6, 7]


def test_the_large_grid_takes_two_grid_rows():
    """1025 x 1024 pairs against 2^20 pairs per grid row: gridDim = (2^20, 2) and the last row
    holds 1024 live pairs; both id lists hit every graph of b10."""
    assert BK.BIG_M * BK.BIG_N > BK.GRID_X == 1 << 20
    assert BK.grid_rows(BK.BIG_M, BK.BIG_N) == (1 << 20, 2, 1024)
    assert BK.grid_rows(13, 13) == (169, 1, 169)
    assert BK.grid_rows(1024, 1024) == (1 << 20, 1, 1 << 20)
    q, db = BK.big_ids()
    G = len(BC.graphs('b10'))
    assert q.shape == (BK.BIG_M,) and db.shape == (BK.BIG_N,) and BK.BIG_LD > BK.BIG_N
    assert set(q.tolist()) == set(db.tolist()) == set(range(G))
    # the second grid row is query row 1024: its pairs are all live and not all alike
    assert len({(int(q[1024]), int(b)) for b in db}) == G
    # width 1: at most n1 <= 10 expansions per pair
    _, ref = BC.store('b10')
    ex = ref.grid(range(G), range(G), BK.BIG_WIDTH)[3]
    assert ex.max() <= 10 and (ex > 0).any()
    assert int(q[1024]) == BK.BIG_LAST_Q and (ex[BK.BIG_LAST_Q] > 0).any()
    assert len(set(ref.grid(range(G), range(G), BK.BIG_WIDTH)[0][BK.BIG_LAST_Q].tolist())) > 1
