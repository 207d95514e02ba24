"""numpy restatement of include/siamese_ged.h: the specification sg_ged_grid must equal bit
for bit (ub, lb and the 1->2 assignment), with the same tie rules.

Cost model: node insertion / deletion 1, substitution 0 for equal type and 1 otherwise, edge
insertion / deletion 1, edge substitution 0.  A graph is (types [n], A bool [n][n]) with a zero
diagonal; deg is the row sum of A.
"""
import numpy as np

BIG = 1 << 20
INF = 2 ** 31 - 1


def graph_of_store(store, g):
    """(types, A) of store graph g: nodes a != b share an edge iff adj[g][a][b] != 0."""
    n = int(store.n[g])
    A = np.asarray(store.adj[g, :n, :n]) != 0
    A = A & ~np.eye(n, dtype=bool)
    return np.asarray(store.types[g, :n], dtype=np.int64), A


def cost_matrix(g1, g2, w):
    """The (n1 + n2)² matrix with substitution weight w (1: upper bound, 2: the doubled
    half-edge-cost matrix of the lower bound)."""
    (t1, A1), (t2, A2) = g1, g2
    n1, n2 = len(t1), len(t2)
    d1, d2 = A1.sum(axis=1).astype(np.int64), A2.sum(axis=1).astype(np.int64)
    C = np.zeros((n1 + n2, n1 + n2), dtype=np.int64)
    C[:n1, :n2] = w * (t1[:, None] != t2[None, :]) + np.abs(d1[:, None] - d2[None, :])
    C[:n1, n2:] = BIG
    C[n1:, :n2] = BIG
    C[np.arange(n1), n2 + np.arange(n1)] = w + d1
    C[n1 + np.arange(n2), np.arange(n2)] = w + d2
    return C


def lsap(C):
    """Shortest augmenting paths with potentials: rows enter in index order, the column argmin
    breaks ties to the smallest index, minv is updated on strict <, every loop is counted.
    Returns (p, cost): p[c] the row of column c."""
    C = np.asarray(C, dtype=np.int64)
    N = C.shape[0]
    u = np.zeros(N, dtype=np.int64)
    v = np.zeros(N, dtype=np.int64)
    p = np.full(N, -1, dtype=np.int64)
    cols = np.arange(N)
    for i in range(N):
        minv = np.full(N, INF, dtype=np.int64)
        way = np.full(N, -1, dtype=np.int64)
        used = np.zeros(N, dtype=bool)
        ui, j0, i0, u0 = 0, -1, i, 0
        for _ in range(N):
            cur = C[i0] - u0 - v
            upd = ~used & (cur < minv)
            minv[upd] = cur[upd]
            way[upd] = j0
            key = np.where(used, np.iinfo(np.int64).max, minv * 64 + cols)
            k = int(key.min())
            j1, delta = k % 64, k // 64
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
        for _ in range(N):
            if j0 < 0:
                break
            j1 = int(way[j0])
            p[j0] = i if j1 < 0 else p[j1]
            j0 = j1
        u[i] = ui
    assert int(np.abs(u).max()) < 2 ** 30 and int(np.abs(v).max()) < 2 ** 30   # int32 on the device
    return p, int(u.sum() + v.sum())


def phi_of(p, n1, n2):
    """phi[a] for a < n1: the graph-2 node of graph-1 node a, or -1 (deleted)."""
    phi = np.full(n1, -1, dtype=np.int64)
    for c, r in enumerate(p):
        if 0 <= r < n1:
            phi[r] = c if c < n2 else -1
    return phi


def induced_cost(g1, g2, phi):
    """Cost of the edit path of phi: deletions + insertions + substitutions of different type
    + |E1| + |E2| - 2 (edges of graph 1 whose image is an edge of graph 2)."""
    (t1, A1), (t2, A2) = g1, g2
    n1, n2 = len(t1), len(t2)
    kept = [a for a in range(n1) if phi[a] >= 0]
    dels = n1 - len(kept)
    ins = n2 - len(kept)
    subs = sum(int(t1[a] != t2[phi[a]]) for a in kept)
    e1, e2 = int(A1.sum()) // 2, int(A2.sum()) // 2
    both = sum(1 for a in kept for b in kept if a < b and A1[a, b] and A2[phi[a], phi[b]])
    return dels + ins + subs + e1 + e2 - 2 * both


def upper_bound(g1, g2):
    """(ub(1->2), phi)."""
    p, _ = lsap(cost_matrix(g1, g2, 1))
    phi = phi_of(p, len(g1[0]), len(g2[0]))
    return induced_cost(g1, g2, phi), phi


def lower_bound(g1, g2):
    _, opt = lsap(cost_matrix(g1, g2, 2))
    return (opt + 1) // 2


def bp_pair(g1, g2, both_orders=True):
    """(ub, lb, phi of the 1->2 order)."""
    ub, phi = upper_bound(g1, g2)
    if both_orders:
        ub = min(ub, upper_bound(g2, g1)[0])
    return ub, lower_bound(g1, g2), phi


class GridReference(object):
    """The restatement over a store, each ordered pair of store graphs solved once."""

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

    def grid(self, q_idx, db_idx, both_orders):
        """(ub int32 [m][n], lb int32 [m][n], map int8 [m][n][n_max]); ids outside the store
        or node counts outside [1, n_max] give -1 entries."""
        nm = self.store.n_max
        G = len(self.store.n)
        ok = lambda g: 0 <= g < G and 1 <= int(self.store.n[g]) <= nm   # noqa: E731
        m, n = len(q_idx), len(db_idx)
        ub = np.full((m, n), -1, dtype=np.int32)
        lb = np.full((m, n), -1, dtype=np.int32)
        mp = np.full((m, n, nm), -1, dtype=np.int8)
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
