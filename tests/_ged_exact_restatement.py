"""Plain-Python restatement of include/siamese_ged_exact.h: the specification sg_ged_exact_grid
must equal bit for bit (ub, lb, map and the expansion count), with the same order rules.

The bipartite seed is tests/_ged_restatement.py's.  A graph is that module's (types [n], A bool
[n][n]); the search works on the row bit masks of A.
"""
from collections import Counter

import numpy as np

import _ged_restatement as R

MAX_SEARCH_NODES = 16
MAX_BUDGET = 1 << 24


def invert(phi21, n1):
    """phi of graph 1 -> graph 2 from the 2->1 assignment: the b with phi21[b] == a, or -1."""
    phi = [-1] * n1
    for b, a in enumerate(phi21):
        if a >= 0:
            phi[int(a)] = b
    return phi


def seed(g1, g2):
    """(ub, lb, phi): sg_ged_grid's both_orders ub and lb, and the graph 1 -> graph 2 map of
    the edit path that costs ub (the 1->2 assignment unless the 2->1 one is strictly cheaper,
    then that one's inverse)."""
    ub12, phi12 = R.upper_bound(g1, g2)
    ub21, phi21 = R.upper_bound(g2, g1)
    lb = R.lower_bound(g1, g2)
    if ub21 < ub12:
        return ub21, lb, invert(phi21, len(g1[0]))
    return ub12, lb, [int(x) for x in phi12]


class _Pair(object):
    """Row masks, types and edge counts of the two graphs."""

    def __init__(self, g1, g2):
        (t1, A1), (t2, A2) = g1, g2
        self.n1, self.n2 = len(t1), len(t2)
        self.t1, self.t2 = [int(x) for x in t1], [int(x) for x in t2]
        self.m1 = [sum(1 << b for b in range(self.n1) if A1[a, b]) for a in range(self.n1)]
        self.m2 = [sum(1 << b for b in range(self.n2) if A2[a, b]) for a in range(self.n2)]
        self.E1 = sum(bin(x).count('1') for x in self.m1) // 2
        self.E2 = sum(bin(x).count('1') for x in self.m2) // 2

    def step(self, phi, c):
        """Cost of mapping graph-1 node k = len(phi) to graph-2 node c (c == n2: to epsilon)
        given phi of the nodes before it: a type mismatch or a deletion 1, every relation to an
        earlier node that disagrees 1."""
        k = len(phi)
        if c == self.n2:
            return 1 + sum((self.m1[k] >> a) & 1 for a in range(k))
        cost = int(self.t1[k] != self.t2[c])
        for a in range(k):
            e1 = (self.m1[k] >> a) & 1
            e2 = (self.m2[c] >> phi[a]) & 1 if phi[a] >= 0 else 0
            cost += int(e1 != e2)
        return cost

    def h(self, k, used):
        """Admissible bound for graph-1 nodes k .. n1-1 against the unused graph-2 nodes:
        max(r1, r2) - |multiset intersection of their types|, plus |e1r - e2r| with e.r the
        edges that have at least one unprocessed (unused) end."""
        rem2 = [j for j in range(self.n2) if not (used >> j) & 1]
        r1, r2 = self.n1 - k, len(rem2)
        common = sum((Counter(self.t1[k:]) & Counter(self.t2[j] for j in rem2)).values())
        low = (1 << k) - 1
        in1 = sum(bin(self.m1[a] & low).count('1') for a in range(k)) // 2
        in2 = sum(bin(self.m2[j] & used).count('1') for j in range(self.n2)
                  if (used >> j) & 1) // 2
        return max(r1, r2) - common + abs((self.E1 - in1) - (self.E2 - in2))


class _Cut(Exception):
    pass


def search(g1, g2, incumbent, budget=None, on_expand=None):
    """Depth-first branch and bound from an incumbent cost.  Returns (proven, expansions,
    improvements): improvements is the list of (expansion number, cost, phi) of every new
    incumbent, in order.  budget None: unlimited."""
    P = _Pair(g1, g2)
    n1, n2 = P.n1, P.n2
    state = dict(exp=0, inc=incumbent)
    log = []
    phi = []

    def visit(k, g, used):
        if budget is not None and state['exp'] == budget:
            raise _Cut()
        state['exp'] += 1
        children = []
        for c in list(j for j in range(n2) if not (used >> j) & 1) + [n2]:
            gc = g + P.step(phi, c)
            hc = P.h(k + 1, used | (1 << c) if c < n2 else used)
            children.append((gc + hc, c, gc))
        if on_expand is not None:
            on_expand(k, list(phi), g, children)
        children.sort()                      # ascending f, ties to the smaller index, eps last
        for f, c, gc in children:
            if f >= state['inc']:
                break
            if k == n1 - 1:                  # h of a complete map is its leaf cost: f is exact
                state['inc'] = f
                log.append((state['exp'], f, phi + [c if c < n2 else -1]))
            else:
                phi.append(c if c < n2 else -1)
                visit(k + 1, gc, used | (1 << c) if c < n2 else used)
                phi.pop()

    try:
        visit(0, 0, 0)
        proven = True
    except _Cut:
        proven = False
    return proven, state['exp'], log


def searched(g1, g2, ub, lb, budget):
    return not (lb == ub or max(len(g1[0]), len(g2[0])) > MAX_SEARCH_NODES or budget == 0)


def exact_pair(g1, g2, budget):
    """(ub, lb, phi, expansions) as sg_ged_exact_grid returns them; budget None: unlimited."""
    ub, lb, phi = seed(g1, g2)
    if not searched(g1, g2, ub, lb, budget):
        return ub, lb, phi, 0
    proven, exp, log = search(g1, g2, ub, budget)
    if log:
        ub, phi = log[-1][1], log[-1][2]
    return ub, (ub if proven else lb), phi, exp


def at_budget(seeded, run, budget):
    """The result at `budget` from one longer run (seeded = seed(...), run = search(...) with a
    budget >= this one, or unlimited): the search is deterministic, so a smaller budget returns
    the incumbent the longer run held after that many expansions."""
    ub, lb, phi = seeded
    proven, exp, log = run
    if budget == 0:
        return ub, lb, phi, 0
    if not (proven and exp <= budget):
        assert exp >= budget
        proven, exp = False, budget
    for e, cost, p in log:
        if e <= budget:
            ub, phi = cost, p
    return ub, (ub if proven else lb), phi, exp


class ExactGridReference(object):
    """The restatement over a store: each ordered pair of store graphs is searched once, at
    the largest budget asked for so far, and smaller budgets are read off that run."""

    def __init__(self, store):
        self.store = store
        self.graphs = {}
        self.seeds = {}
        self.runs = {}

    def graph(self, g):
        if g not in self.graphs:
            self.graphs[g] = R.graph_of_store(self.store, g)
        return self.graphs[g]

    def pair(self, a, b, budget):
        g1, g2 = self.graph(a), self.graph(b)
        if (a, b) not in self.seeds:
            self.seeds[(a, b)] = seed(g1, g2)
        s = self.seeds[(a, b)]
        if not searched(g1, g2, s[0], s[1], budget):
            return s + (0,)
        have = self.runs.get((a, b))
        if have is None or not (have[1][0] or have[0] >= budget):
            have = (budget, search(g1, g2, s[0], budget))
            self.runs[(a, b)] = have
        return at_budget(s, have[1], budget)

    def grid(self, q_idx, db_idx, budget):
        """(ub int32 [m][n], lb int32 [m][n], map int8 [m][n][n_max], expansions int64 [m][n]);
        ids outside the store or node counts outside [1, n_max] give -1 entries."""
        nm = self.store.n_max
        G = len(self.store.n)
        ok = lambda g: 0 <= g < G and 1 <= int(self.store.n[g]) <= nm   # noqa: E731
        m, n = len(q_idx), len(db_idx)
        ub = np.full((m, n), -1, dtype=np.int32)
        lb = np.full((m, n), -1, dtype=np.int32)
        mp = np.full((m, n, nm), -1, dtype=np.int8)
        ex = np.full((m, n), -1, dtype=np.int64)
        for i, a in enumerate(q_idx):
            for j, b in enumerate(db_idx):
                a, b = int(a), int(b)
                if not (ok(a) and ok(b)):
                    continue
                u, l, phi, e = self.pair(a, b, budget)
                ub[i, j], lb[i, j], ex[i, j] = u, l, e
                mp[i, j, :len(phi)] = phi
        return ub, lb, mp, ex
