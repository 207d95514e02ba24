"""Plain-Python restatement of include/siamese_ged_refine.h: the specification sg_ged_refine_grid
must equal bit for bit (ub, lb, map and the accepted-move count), with the same order rules.

The seed is tests/_ged_restatement.py's (both assignment orders and the lower bound) with
tests/_ged_exact_restatement.py's inversion of the 2->1 map; a graph is that module's (types
[n], A bool [n][n]).  A move's cost is computed as a difference from the current cost, as the
kernel does; tests/test_ged_refine_host.py checks every accepted move against induced_cost.
"""
import numpy as np

import _ged_exact_restatement as X
import _ged_restatement as R

MAX_MOVES = 4096
KINDS = ('exchange', 'free', 'undelete', 'handover')


def seeds(g1, g2):
    """((ub12, phi12), (ub21, inverse of phi21), lb): the two starts and the lower bound."""
    ub12, phi12 = R.upper_bound(g1, g2)
    ub21, phi21 = R.upper_bound(g2, g1)
    return ((ub12, [int(x) for x in phi12]), (ub21, X.invert(phi21, len(g1[0]))),
            R.lower_bound(g1, g2))


def _popc(x):
    return bin(x).count('1')


def kind_of(y, b):
    """The kind of a move from the old image y of a and the node b that held x (or -1 each)."""
    if b >= 0:
        return 'exchange' if y >= 0 else 'handover'
    return 'free' if y >= 0 else 'undelete'


def descend(g1, g2, phi, cost):
    """The whole descent of one start, without a move limit (every accepted move lowers the
    cost, so it ends): the list of (cost, phi, a, x, kind) after each accepted move."""
    P = X._Pair(g1, g2)
    n1, n2, t1, t2, m1, m2 = P.n1, P.n2, P.t1, P.t2, P.m1, P.m2
    phi = list(phi)
    inv = [-1] * n2
    for a, y in enumerate(phi):
        if y >= 0:
            inv[y] = a
    path = []
    while True:
        # per graph-1 node the images of its neighbours
        img = [sum(1 << phi[c] for c in range(n1) if (m1[a] >> c) & 1 and phi[c] >= 0)
               for a in range(n1)]
        best = None
        for a in range(n1):
            y = phi[a]
            for x in range(n2):
                if x == y:
                    continue
                b = inv[x]
                ym, bm = y >= 0, b >= 0
                both = ym and bm
                dnk = 1 + int(both) - int(ym) - int(bm)
                dsub = int(t1[a] != t2[x])
                kept = _popc(img[a] & m2[x])
                if ym:
                    dsub -= int(t1[a] != t2[y])
                    kept -= _popc(img[a] & m2[y])
                if bm:
                    dsub -= int(t1[b] != t2[x])
                    kept -= _popc(img[b] & m2[x])
                if both:
                    dsub += int(t1[b] != t2[y])
                    kept += _popc(img[b] & m2[y])
                    if (m1[a] >> b) & 1 and (m2[x] >> y) & 1:
                        kept += 2      # the a-b edge: counted at both ends before, at neither after
                key = (cost - 2 * dnk + dsub - 2 * kept, a, x)
                if best is None or key < best:
                    best = key
        if best is None or best[0] >= cost:
            return path
        cost, a, x = best
        y, b = phi[a], inv[x]
        phi[a], inv[x] = x, a
        if b >= 0:
            phi[b] = y
        if y >= 0:
            inv[y] = b
        path.append((cost, list(phi), a, x, kind_of(y, b)))


def at_budget(start, path, max_moves):
    """(cost, phi, moves) of a start limited to max_moves accepted moves."""
    k = min(len(path), max_moves)
    if k == 0:
        return start[0], start[1], 0
    return path[k - 1][0], path[k - 1][1], k


def searched(s, max_moves):
    return not (s[2] == min(s[0][0], s[1][0]) or max_moves == 0)


def result(s, paths, max_moves):
    """(ub, lb, phi, moves) from the seeds and both starts' whole descents."""
    if not searched(s, max_moves):
        paths, max_moves = ([], []), 0
    c0, p0, k0 = at_budget(s[0], paths[0], max_moves)
    c1, p1, k1 = at_budget(s[1], paths[1], max_moves)
    ub, phi = (c1, p1) if c1 < c0 else (c0, p0)
    return ub, s[2], list(phi), k0 + k1


def refine_pair(g1, g2, max_moves):
    """(ub, lb, phi, moves) as sg_ged_refine_grid returns them."""
    s = seeds(g1, g2)
    paths = ([], [])
    if searched(s, max_moves):
        paths = tuple(descend(g1, g2, s[k][1], s[k][0]) for k in (0, 1))
    return result(s, paths, max_moves)


class RefineGridReference(object):
    """The restatement over a store: each ordered pair of store graphs descends once from both
    starts, and every budget is read off those descents."""

    def __init__(self, store):
        self.store = store
        self.graphs = {}
        self.seeds = {}
        self.paths = {}

    def graph(self, g):
        if g not in self.graphs:
            self.graphs[g] = R.graph_of_store(self.store, g)
        return self.graphs[g]

    def seed(self, a, b):
        if (a, b) not in self.seeds:
            self.seeds[(a, b)] = seeds(self.graph(a), self.graph(b))
        return self.seeds[(a, b)]

    def descents(self, a, b):
        """Both starts' whole descents; of a pair the seed already proves, none."""
        if (a, b) not in self.paths:
            s = self.seed(a, b)
            self.paths[(a, b)] = ([], []) if not searched(s, MAX_MOVES) else tuple(
                descend(self.graph(a), self.graph(b), s[k][1], s[k][0]) for k in (0, 1))
        return self.paths[(a, b)]

    def pair(self, a, b, max_moves):
        return result(self.seed(a, b), self.descents(a, b), max_moves)

    def grid(self, q_idx, db_idx, max_moves):
        """(ub int32 [m][n], lb int32 [m][n], map int8 [m][n][n_max], moves int32 [m][n]); ids
        outside the store or node counts outside [1, n_max] give -1 entries."""
        nm = self.store.n_max
        G = len(self.store.n)
        ok = lambda g: 0 <= g < G and 1 <= int(self.store.n[g]) <= nm   # noqa: E731
        m, n = len(q_idx), len(db_idx)
        ub = np.full((m, n), -1, dtype=np.int32)
        lb = np.full((m, n), -1, dtype=np.int32)
        mp = np.full((m, n, nm), -1, dtype=np.int8)
        mv = np.full((m, n), -1, dtype=np.int32)
        for i, a in enumerate(q_idx):
            for j, b in enumerate(db_idx):
                a, b = int(a), int(b)
                if not (ok(a) and ok(b)):
                    continue
                u, l, phi, k = self.pair(a, b, max_moves)
                ub[i, j], lb[i, j], mv[i, j] = u, l, k
                mp[i, j, :len(phi)] = phi
        return ub, lb, mp, mv
