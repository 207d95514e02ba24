"""numpy restatement of include/siamese_ged_csr.h: the specification sg_csr_ged_grid must equal
bit for bit (ub, lb and the 1->2 assignment), with the same tie rules, read from the arrays of a
web.CsrStore.  No lane count appears here: the argmin is over (minv, column) pairs.  Every solve
asserts the header's integer bounds.

Cost model: node insertion / deletion 1, substitution 0 for equal type and 1 otherwise, edge
insertion / deletion 1, edge substitution 0.  A graph is (types [n], A bool [n][n]) with a zero
diagonal: A[a][b] iff the store holds an entry (a, b), a != b, with val != 0.
"""
import numpy as np

F = 1 << 21                  # forbidden entries
INF = 2 ** 31 - 1
K = 2 + 511                  # the largest finite entry
D = 1024 * K                 # the largest optimum, distance and |v|


def graph_of_store(store, g):
    off, n = int(store.node_off[g]), int(store.n[g])
    A = np.zeros((n, n), dtype=bool)
    for a in range(n):
        s0, s1 = int(store.row_ptr[off + a]), int(store.row_ptr[off + a + 1])
        cols = np.asarray(store.col[s0:s1])
        assert (np.diff(cols) > 0).all()                  # strictly ascending
        A[a, cols[np.asarray(store.val[s0:s1]) != 0]] = True
    A &= ~np.eye(n, dtype=bool)
    assert np.array_equal(A, A.T)
    return np.asarray(store.types[off:off + n], dtype=np.int64), A


def cost_matrix(g1, g2, w):
    (t1, A1), (t2, A2) = g1, g2
    n1, n2 = len(t1), len(t2)
    d1, d2 = A1.sum(axis=1).astype(np.int64), A2.sum(axis=1).astype(np.int64)
    C = np.zeros((n1 + n2, n1 + n2), dtype=np.int64)
    C[:n1, :n2] = w * (t1[:, None] != t2[None, :]) + np.abs(d1[:, None] - d2[None, :])
    C[:n1, n2:] = F
    C[n1:, :n2] = F
    C[np.arange(n1), n2 + np.arange(n1)] = w + d1
    C[n1 + np.arange(n2), np.arange(n2)] = w + d2
    return C


def lsap(C, count=None):
    """Shortest augmenting paths with potentials: rows enter in index order, a round takes the
    unmarked column of smallest minv, ties to the smallest index, minv is replaced on strict <,
    every loop is counted.  Returns (p, cost): p[c] the row of column c.  count: a one-element
    list that receives the number of rounds."""
    C = np.asarray(C, dtype=np.int64)
    N = C.shape[0]
    assert N <= 1024
    u = np.zeros(N, dtype=np.int64)
    v = np.zeros(N, dtype=np.int64)
    p = np.full(N, -1, dtype=np.int64)
    rounds = 0
    for i in range(N):
        minv = np.full(N, INF, dtype=np.int64)
        way = np.full(N, -1, dtype=np.int64)
        used = np.zeros(N, dtype=bool)
        ui, j0, i0, u0 = 0, -1, i, 0
        for _ in range(N):
            rounds += 1
            cur = C[i0] - u0 - v
            upd = ~used & (cur < minv)
            minv[upd] = cur[upd]
            way[upd] = j0
            open_ = np.flatnonzero(~used)
            mo = minv[open_]
            assert int(mo.min()) >= 0 and int(mo.max()) <= F + D < 1 << 22    # the uint32 key
            delta = int(mo.min())
            j1 = int(open_[np.argmax(mo == delta)])       # (minv, column) lexicographic
            assert delta <= D                             # far below a forbidden entry's minv
            v[used] -= delta
            u[p[used]] += delta
            minv[~used] -= delta
            ui += delta
            j0 = j1
            used[j0] = True
            i0 = int(p[j0])
            if i0 < 0:
                break
            u0 = int(u[i0])
        assert 0 <= ui <= D
        for _ in range(N):
            if j0 < 0:
                break
            j1 = int(way[j0])
            p[j0] = i if j1 < 0 else p[j1]
            j0 = j1
        u[i] = ui
        assert int(v.min()) >= -D and int(v.max()) <= 0
        assert int(u.min()) >= 0 and int(u.max()) <= K + D
    assert (C[p, np.arange(N)] < F).all()
    if count is not None:
        count[0] = rounds
    cost = int(u.sum() + v.sum())
    assert 0 <= cost <= D
    return p, cost


def phi_of(p, n1, n2):
    phi = np.full(n1, -1, dtype=np.int64)
    for c, r in enumerate(p):
        if 0 <= r < n1:
            phi[r] = c if c < n2 else -1
    return phi


def induced_cost(g1, g2, phi):
    """deletions + insertions + substitutions of different type + |E1| + |E2| - 2 (edges of
    graph 1 whose image is an edge of graph 2)."""
    (t1, A1), (t2, A2) = g1, g2
    n1, n2 = len(t1), len(t2)
    phi = np.asarray(phi)
    kept = np.flatnonzero(phi >= 0)
    dels, ins = n1 - kept.size, n2 - kept.size
    subs = int((t1[kept] != t2[phi[kept]]).sum())
    e1, e2 = int(A1.sum()) // 2, int(A2.sum()) // 2
    both = int((A1[np.ix_(kept, kept)] & A2[np.ix_(phi[kept], phi[kept])]).sum()) // 2
    return dels + ins + subs + e1 + e2 - 2 * both


def upper_bound(g1, g2):
    p, _ = lsap(cost_matrix(g1, g2, 1))
    phi = phi_of(p, len(g1[0]), len(g2[0]))
    return induced_cost(g1, g2, phi), phi


def lower_bound(g1, g2):
    _, opt = lsap(cost_matrix(g1, g2, 2))
    return (opt + 1) // 2


class GridReference(object):
    """The restatement over a CsrStore, each ordered pair of store graphs solved once."""

    def __init__(self, store):
        self.store = store
        self.graphs = {}
        self.pairs = {}

    def graph(self, g):
        if g not in self.graphs:
            self.graphs[g] = graph_of_store(self.store, g)
        return self.graphs[g]

    def pair(self, a, b):
        """(ub(a->b), lb, phi) without the min over orders."""
        if (a, b) not in self.pairs:
            ub, phi = upper_bound(self.graph(a), self.graph(b))
            self.pairs[(a, b)] = (ub, lower_bound(self.graph(a), self.graph(b)), phi)
        return self.pairs[(a, b)]

    def grid(self, q_idx, db_idx, both_orders, n_max=None):
        """(ub int32 [m][n], lb int32 [m][n], map int16 [m][n][n_max]); ids outside the store
        or node counts outside [1, n_max] give -1 entries."""
        nm = self.store.n_max if n_max is None else n_max
        G = len(self.store.n)
        ok = lambda g: 0 <= g < G and 1 <= int(self.store.n[g]) <= nm   # noqa: E731
        m, n = len(q_idx), len(db_idx)
        ub = np.full((m, n), -1, dtype=np.int32)
        lb = np.full((m, n), -1, dtype=np.int32)
        mp = np.full((m, n, nm), -1, dtype=np.int16)
        for i, a in enumerate(q_idx):
            for j, b in enumerate(db_idx):
                a, b = int(a), int(b)
                if not (ok(a) and ok(b)):
                    continue
                u, l, phi = self.pair(a, b)
                if both_orders:
                    u = min(u, self.pair(b, a)[0])
                ub[i, j], lb[i, j] = u, l
                mp[i, j, :len(phi)] = phi
        return ub, lb, mp
