"""Plain-Python restatement of include/siamese_mcs.h: the specification sg_mcs_grid must equal
bit for bit (size, bound, map, edges and the expansion count), with the same order rules.

A graph is tests/_ged_restatement.py's (types [n], A bool [n][n]); the search works on the row
bit masks of A.  A class is (L, R, adj) with L and R as bit sets.
"""
import numpy as np

import _ged_restatement as R

MAX_BUDGET = 1 << 24


def _pc(x):
    return bin(x).count('1')


def _masks(g):
    t, A = g
    n = len(t)
    return n, [int(x) for x in t], [sum(1 << b for b in range(n) if A[a, b]) for a in range(n)]


def root_classes(g1, g2):
    """One class per type of both graphs, in the order of the type's smallest graph-1 node."""
    (n1, t1, _), (n2, t2, _) = _masks(g1), _masks(g2)
    classes, seen = [], set()
    for a in range(n1):
        if t1[a] in seen:
            continue
        seen.add(t1[a])
        L = sum(1 << x for x in range(n1) if t1[x] == t1[a])
        Rs = sum(1 << x for x in range(n2) if t2[x] == t1[a])
        if Rs:
            classes.append((L, Rs, 0))
    return classes


def _rest(classes):
    return sum(min(_pc(L), _pc(Rs)) for L, Rs, _ in classes)


class _Stop(Exception):
    pass


TRACE_KEYS = ('classes_expanded', 'classes_child', 'level', 'no_class')


def search(g1, g2, connected, budget=None, trace=None):
    """Depth-first McSplit from the root.  Returns (proven, expansions, ub0, improvements):
    improvements is the list of (expansion number, size, phi) of every new incumbent, in order.
    budget None: unlimited.

    trace: a dict that receives what the search reached, and changes no result: the largest class
    count of an expanded state ('classes_expanded') and of a generated child, expanded or not
    ('classes_child'), the deepest level expanded ('level', the root is level 0) and the number
    of expansions that found no class to select ('no_class').  Maxima and the count accumulate
    over the calls that share a dict."""
    (n1, _, N1), (n2, _, N2) = _masks(g1), _masks(g2)
    root = root_classes(g1, g2)
    ub0 = _rest(root)
    st = dict(exp=0, inc=0, proven=False)
    log = []

    def note(key, value, add=False):
        if trace is not None:
            trace[key] = trace.get(key, 0) + value if add else max(trace.get(key, 0), value)

    def expand(M, classes, level):
        if budget is not None and st['exp'] == budget:
            raise _Stop()
        st['exp'] += 1
        note('classes_expanded', len(classes))
        note('level', level)
        cand = [(max(_pc(c[0]), _pc(c[1])), i) for i, c in enumerate(classes)
                if not (connected and M) or c[2]]
        if not cand:
            note('no_class', 1, add=True)
            return
        i = min(cand)[1]                      # smallest max(|L|, |R|), ties to the earliest
        L, Rs, adj = classes[i]
        v = (L & -L).bit_length() - 1
        for w in [w for w in range(n2) if (Rs >> w) & 1] + [None]:
            if st['inc'] == ub0:
                st['proven'] = True
                raise _Stop()
            if w is None:                     # v unmatched, last
                M2 = M
                L2 = L & ~(1 << v)
                child = classes[:i] + ([(L2, Rs, adj)] if L2 else []) + classes[i + 1:]
            else:
                M2 = M + [(v, w)]
                child = []
                for l, r, a in classes:
                    l &= ~(1 << v)
                    r &= ~(1 << w)
                    if l & N1[v] and r & N2[w]:
                        child.append((l & N1[v], r & N2[w], 1))
                    if l & ~N1[v] and r & ~N2[w]:
                        child.append((l & ~N1[v], r & ~N2[w], a))
                if len(M2) > st['inc']:
                    st['inc'] = len(M2)
                    phi = [-1] * n1
                    for a, b in M2:
                        phi[a] = b
                    log.append((st['exp'], len(M2), phi))
            note('classes_child', len(child))
            if len(M2) + _rest(child) > st['inc']:
                expand(M2, child, level + 1)

    if trace is not None:
        for key in TRACE_KEYS:
            trace.setdefault(key, 0)
    if ub0 == 0:
        return True, 0, 0, log
    try:
        expand([], root, 0)
        st['proven'] = True
    except _Stop:
        pass
    return st['proven'], st['exp'], ub0, log


def edges_of(g1, phi):
    _, A = g1
    n1 = len(phi)
    return sum(1 for a in range(n1) for c in range(a) if A[a, c] and phi[a] >= 0 and phi[c] >= 0)


def at_budget(g1, run, budget):
    """(size, bound, phi, edges, expansions) at `budget` from one longer run (a search with a
    budget >= this one, or unlimited): the search is deterministic, so a smaller budget returns
    the incumbent the longer run held after that many expansions."""
    proven, exp, ub0, log = run
    n1 = len(g1[0])
    if budget is not None and not (proven and exp <= budget):
        assert exp >= budget
        proven, exp = False, budget
    size, phi = 0, [-1] * n1
    for e, s, p in log:
        if e <= exp:
            size, phi = s, p
    return size, (size if proven else ub0), phi, edges_of(g1, phi), exp


def mcs_pair(g1, g2, connected, budget):
    """(size, bound, map, edges, expansions) as sg_mcs_grid returns them; budget None:
    unlimited."""
    return at_budget(g1, search(g1, g2, connected, budget), budget)


class McsGridReference(object):
    """The restatement over a store: each ordered pair of store graphs is searched once per
    `connected`, at the largest budget asked for so far, and smaller budgets are read off that
    run."""

    def __init__(self, store):
        self.store = store
        self.graphs = {}
        self.runs = {}
        self.trace = {}          # what all its searches reached (search's trace)

    def graph(self, g):
        if g not in self.graphs:
            self.graphs[g] = R.graph_of_store(self.store, g)
        return self.graphs[g]

    def pair(self, a, b, connected, budget):
        g1, g2 = self.graph(a), self.graph(b)
        key = (a, b, bool(connected))
        have = self.runs.get(key)
        if have is None or not (have[1][0] or have[0] is None or
                                (budget is not None and have[0] >= budget)):
            have = (budget, search(g1, g2, bool(connected), budget, trace=self.trace))
            self.runs[key] = have
        return at_budget(g1, have[1], budget)

    def grid(self, q_idx, db_idx, connected, budget):
        """(size int32 [m][n], bound int32 [m][n], map int8 [m][n][n_max], edges int32 [m][n],
        expansions int64 [m][n]); ids outside the store or node counts outside [1, n_max] give
        -1 entries."""
        nm = self.store.n_max
        G = len(self.store.n)
        ok = lambda g: 0 <= g < G and 1 <= int(self.store.n[g]) <= nm   # noqa: E731
        m, n = len(q_idx), len(db_idx)
        size = np.full((m, n), -1, dtype=np.int32)
        bound = np.full((m, n), -1, dtype=np.int32)
        mp = np.full((m, n, nm), -1, dtype=np.int8)
        ed = np.full((m, n), -1, dtype=np.int32)
        ex = np.full((m, n), -1, dtype=np.int64)
        for i, a in enumerate(q_idx):
            for j, b in enumerate(db_idx):
                a, b = int(a), int(b)
                if not (ok(a) and ok(b)):
                    continue
                s, bd, phi, e, x = self.pair(a, b, connected, budget)
                size[i, j], bound[i, j], ed[i, j], ex[i, j] = s, bd, e, x
                mp[i, j, :len(phi)] = phi
        return size, bound, mp, ed, ex
