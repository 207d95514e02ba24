"""Plain-Python restatement of include/siamese_ged_beam.h: the specification sg_ged_beam_grid
must equal bit for bit (ub, lb, map and the expanded count), with the same order rules.

The seed, the step cost and h are tests/_ged_exact_restatement.py's (imported, not copied); a
graph is tests/_ged_restatement.py's (types [n], A bool [n][n]).
"""
import numpy as np

import _ged_exact_restatement as X
import _ged_restatement as R

MAX_WIDTH = 128


def search(g1, g2, incumbent, width=None):
    """The level-synchronous beam from an incumbent cost; width None: no limit (a complete
    search).  Returns (truncated, expanded, leaf, survivors): leaf is (cost, phi) of the first
    complete map below the incumbent or None, survivors the number of children that survived
    the pruning at each level reached."""
    P = X._Pair(g1, g2)
    n1, n2 = P.n1, P.n2
    hmemo = {}

    def h(k, used):
        if (k, used) not in hmemo:
            hmemo[(k, used)] = P.h(k, used)
        return hmemo[(k, used)]

    level = [(0, 0, [])]                      # (g, used, phi) by slot
    expanded, truncated, survivors = 0, False, []
    for k in range(n1):
        children = []
        for p, (g, used, phi) in enumerate(level):
            expanded += 1
            for c in [j for j in range(n2) if not (used >> j) & 1] + [n2]:
                gc = g + P.step(phi, c)
                uc = used | (1 << c) if c < n2 else used
                f = gc + h(k + 1, uc)
                if f < incumbent:             # pruning, not truncation
                    children.append((f, p, c, gc, uc))
        survivors.append(len(children))
        children.sort()                       # f, then parent slot, then index with eps last
        if not children:
            return truncated, expanded, None, survivors
        if k == n1 - 1:
            f, p, c = children[0][:3]
            return truncated, expanded, (f, level[p][2] + [c if c < n2 else -1]), survivors
        if width is not None and len(children) > width:
            truncated = True
            children = children[:width]
        level = [(gc, uc, level[p][2] + [c if c < n2 else -1]) for f, p, c, gc, uc in children]
    raise AssertionError('n1 >= 1 levels')


def searched(ub, lb, width):
    return not (lb == ub or width == 0)


def beam_pair(g1, g2, width, seeded=None):
    """(ub, lb, phi, expanded) as sg_ged_beam_grid returns them; width None: no limit."""
    ub, lb, phi = seeded if seeded is not None else X.seed(g1, g2)
    if not searched(ub, lb, width):
        return ub, lb, phi, 0
    truncated, expanded, leaf, _ = search(g1, g2, ub, width)
    if leaf is not None:
        ub, phi = leaf
    return ub, (lb if truncated else ub), phi, expanded


def is_truncated(g1, g2, width, seeded=None):
    """Whether the pair's search runs at this width and drops a state because of it."""
    ub, lb, _ = seeded if seeded is not None else X.seed(g1, g2)
    return searched(ub, lb, width) and search(g1, g2, ub, width)[0]


class BeamGridReference(object):
    """The restatement over a store, each (ordered pair of store graphs, width) searched once."""

    def __init__(self, store):
        self.store = store
        self.graphs = {}
        self.seeds = {}
        self.runs = {}
        self.whole = {}
        self.survivors = {}      # of the runs made: the children left by the pruning, by level

    def graph(self, g):
        if g not in self.graphs:
            self.graphs[g] = R.graph_of_store(self.store, g)
        return self.graphs[g]

    def seed(self, a, b):
        if (a, b) not in self.seeds:
            self.seeds[(a, b)] = X.seed(self.graph(a), self.graph(b))
        return self.seeds[(a, b)]

    def run(self, a, b, width):
        """((ub, lb, phi, expanded), truncated).  A width that cut no level cuts none at any
        larger width either, so that run is the result of every larger width as well."""
        s = self.seed(a, b)
        if not searched(s[0], s[1], width):
            return s + (0,), False
        if (a, b) in self.whole and width >= self.whole[(a, b)][0]:
            return self.whole[(a, b)][1], False
        if (a, b, width) not in self.runs:
            g1, g2 = self.graph(a), self.graph(b)
            truncated, expanded, leaf, survivors = search(g1, g2, s[0], width)
            self.survivors[(a, b, width)] = survivors
            ub, phi = leaf if leaf is not None else (s[0], s[2])
            self.runs[(a, b, width)] = ((ub, s[1] if truncated else ub, phi, expanded), truncated)
            if not truncated:
                self.whole[(a, b)] = (width, self.runs[(a, b, width)][0])
        return self.runs[(a, b, width)]

    def pair(self, a, b, width):
        return self.run(a, b, width)[0]

    def grid(self, q_idx, db_idx, width):
        """(ub int32 [m][n], lb int32 [m][n], map int8 [m][n][n_max], expanded int32 [m][n]);
        ids outside the store or node counts outside [1, n_max] give -1 entries."""
        nm = self.store.n_max
        G = len(self.store.n)
        ok = lambda g: 0 <= g < G and 1 <= int(self.store.n[g]) <= nm   # noqa: E731
        m, n = len(q_idx), len(db_idx)
        ub = np.full((m, n), -1, dtype=np.int32)
        lb = np.full((m, n), -1, dtype=np.int32)
        mp = np.full((m, n, nm), -1, dtype=np.int8)
        ex = np.full((m, n), -1, dtype=np.int32)
        for i, a in enumerate(q_idx):
            for j, b in enumerate(db_idx):
                a, b = int(a), int(b)
                if not (ok(a) and ok(b)):
                    continue
                u, l, phi, e = self.pair(a, b, width)
                ub[i, j], lb[i, j], ex[i, j] = u, l, e
                mp[i, j, :len(phi)] = phi
        return ub, lb, mp, ex
