"""Plain-Python restatement of include/siamese_ged_knn.h: the specification sg_ged_knn must
equal bit for bit (columns, ub, lb, the certificate, the candidate count and the expansions of
every row), in the header's five steps: seed, threshold, filter, verify, select.

The seed and the search are tests/_ged_exact_restatement.py's; the search takes its incumbent
as an argument, which is all the cutoff needs.
"""
import numpy as np

import _ged_exact_restatement as X

MAX_K = 64


def verify_outcome(ub0, lb0, c, at):
    """(ub, lb, expansions) of a searched candidate from X.at_budget's (ub, lb, phi, exp) of the
    run that started at incumbent c: a map was found iff its cost lies below c."""
    ub, lb, _, exp = at
    ended = lb == ub
    if ub < c:                                # a complete map was found
        return ub, (ub if ended else lb0), exp
    if not ended:                             # the budget ended it
        return ub0, lb0, exp
    if c == ub0:                              # proven: nothing cheaper than the seed
        return ub0, ub0, exp
    return ub0, max(lb0, c), exp              # proven outside the threshold


class KnnReference(object):
    """The restatement over a store.  A pair's run depends on the two graphs, the cutoff and
    the budget alone, so each (a, b, c) is searched once at the largest budget asked for and
    smaller budgets are read off that run, as X.ExactGridReference does for c == ub0."""

    def __init__(self, store, exact=None):
        self.store = store
        self.exact = exact if exact is not None else X.ExactGridReference(store)
        self.runs = {}

    def servable(self, g):
        return 0 <= g < len(self.store.n) and 1 <= int(self.store.n[g]) <= self.store.n_max

    def seed(self, a, b):
        """(ub0, lb0) of sg_ged_grid with both_orders = 1."""
        self.exact.pair(a, b, 0)
        return self.exact.seeds[(a, b)][:2]

    def verify(self, a, b, tau, budget):
        """(ub, lb, expansions, c) of candidate (a, b) under threshold tau."""
        ub0, lb0 = self.seed(a, b)
        c = min(ub0, tau + 1)
        g1, g2 = self.exact.graph(a), self.exact.graph(b)
        if not X.searched(g1, g2, ub0, lb0, budget):
            return ub0, lb0, 0, c
        if c == ub0:                          # sg_ged_exact_grid's pair, bit for bit
            u, l, _, e = self.exact.pair(a, b, budget)
            return u, l, e, c
        have = self.runs.get((a, b, c))
        if have is None or not (have[1][0] or have[0] >= budget):
            have = (budget, X.search(g1, g2, c, budget))
            self.runs[(a, b, c)] = have
        at = X.at_budget((ub0, lb0, None), have[1], budget)
        return verify_outcome(ub0, lb0, c, at) + (c,)

    def row(self, a, db_idx, k, budget):
        """One query: dict(cols, ub, lb [k], certified, candidates, expansions, tau, pairs);
        pairs maps a candidate column to (ub0, lb0, c, ub, lb, expansions)."""
        neg = [-1] * k
        if not self.servable(a):
            return dict(cols=neg, ub=neg, lb=neg, certified=0, candidates=-1, expansions=-1,
                        tau=-1, pairs={})
        valid = [j for j, b in enumerate(db_idx) if self.servable(int(b))]
        kq = min(k, len(valid))
        if kq == 0:
            return dict(cols=neg, ub=neg, lb=neg, certified=1, candidates=0, expansions=0,
                        tau=-1, pairs={})
        seeds = {j: self.seed(a, int(db_idx[j])) for j in valid}
        tau = sorted(s[0] for s in seeds.values())[kq - 1]
        pairs = {}
        for j in valid:
            ub0, lb0 = seeds[j]
            if lb0 <= tau:
                u, l, e, c = self.verify(a, int(db_idx[j]), tau, budget)
                pairs[j] = (ub0, lb0, c, u, l, e)
        order = sorted(pairs, key=lambda j: (pairs[j][3], j))
        sel, rest = order[:kq], order[kq:]
        d, s = pairs[sel[-1]][3], sel[-1]
        cert = all(pairs[j][4] == pairs[j][3] for j in sel) and \
            all(pairs[j][4] > d or (pairs[j][4] == d and j > s) for j in rest)
        pad = [-1] * (k - kq)
        return dict(cols=sel + pad, ub=[pairs[j][3] for j in sel] + pad,
                    lb=[pairs[j][4] for j in sel] + pad, certified=int(cert),
                    candidates=len(pairs), expansions=sum(p[5] for p in pairs.values()),
                    tau=tau, pairs=pairs)

    def rows(self, q_idx, db_idx, k, budget):
        """The rows of a grid: equal queries against one db_idx share a row."""
        db_idx = [int(b) for b in db_idx]
        done = {}
        out = []
        for a in q_idx:
            a = int(a)
            if a not in done:
                done[a] = self.row(a, db_idx, k, budget)
            out.append(done[a])
        return out

    def knn(self, q_idx, db_idx, k, budget):
        """(cols int32 [m][k], ub, lb, certified int32 [m], candidates int32 [m], expansions
        int64 [m]) as sg_ged_knn writes them."""
        rows = self.rows(q_idx, db_idx, k, budget)
        i32 = lambda key: np.array([r[key] for r in rows], dtype=np.int32)   # noqa: E731
        return (i32('cols').reshape(len(rows), k), i32('ub').reshape(len(rows), k),
                i32('lb').reshape(len(rows), k), i32('certified'), i32('candidates'),
                np.array([r['expansions'] for r in rows], dtype=np.int64))


def brute_force_topk(dist_row, k):
    """The first min(k, servable) columns of a row of exact distances (-1: unservable) in
    ascending (distance, column), padded with -1 to k."""
    cols = sorted((j for j, d in enumerate(dist_row) if d >= 0), key=lambda j: (dist_row[j], j))
    cols = cols[:k]
    return cols + [-1] * (k - len(cols))
