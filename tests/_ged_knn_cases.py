"""The graph sets the k-nearest GED tests share (test_ged_knn_host.py proves on the host what
test_gpu_ged_knn.py relies on): cap10, tie10 and cap32 of _ged_exact_cases, and

  knn24  24 random connected graphs of 3 to 9 nodes in a capacity-10 store, drawn like cap10.
         KNN24_SEED was chosen on the host so that the restatement at k = 3 and PROVE_BUDGET
         shows a row with fewer candidates than columns, a pair proven out by the cutoff (lb
         raised to tau + 1 below its ub0), a tie in ub at the k-th place decided by column, and
         every row certified; test_ged_knn_host.py asserts all four.
"""
import numpy as np

import _ged_exact_cases as C
import _ged_knn_restatement as K

PROVE_BUDGET = C.PROVE_BUDGET
CUT_BUDGETS = C.CUT_BUDGETS
SETS = ('cap10', 'tie10', 'cap32', 'knn24')
KNN24_SEED = 2
KNN24_GRAPHS = 24


def graphs(name, seed=None):
    if name != 'knn24':
        return C.graphs(name)
    rng = np.random.default_rng(KNN24_SEED if seed is None else seed)
    sizes = [int(x) for x in rng.integers(3, 10, size=KNN24_GRAPHS)]
    return [C._random_graph(rng, n, i, p_extra=0.15) for i, n in enumerate(sizes)]


_STORES = {}


def store(name):
    """(store, KnnReference) of a named set, built once per process; the three shared sets
    keep _ged_exact_cases' store and exact reference."""
    if name not in _STORES:
        if name == 'knn24':
            from graphembedding_amd.ged import store_of_graphs
            s = store_of_graphs(graphs(name), n_max=10)
            _STORES[name] = (s, K.KnnReference(s))
        else:
            s, exact = C.store(name)
            _STORES[name] = (s, K.KnnReference(s, exact))
    return _STORES[name]


def knn24_properties(ref, k=3, budget=PROVE_BUDGET):
    """(a) rows with fewer candidates than columns, (b) pairs proven out by the cutoff, (c)
    rows whose k-th place is a tie in ub decided by column, (d) rows certified, of all rows of
    the set against the whole set."""
    G = len(ref.store.n)
    rows = ref.rows(range(G), range(G), k, budget)
    fewer = [i for i, r in enumerate(rows) if r['candidates'] < G]
    cut = [(i, j) for i, r in enumerate(rows) for j, p in r['pairs'].items()
           if p[2] == r['tau'] + 1 < p[0] and p[4] == r['tau'] + 1 and p[3] == p[0]]
    tie = []
    for i, r in enumerate(rows):
        d, s = r['ub'][k - 1], r['cols'][k - 1]
        if any(p[3] == d and j > s for j, p in r['pairs'].items()):
            tie.append(i)
    cert = [i for i, r in enumerate(rows) if r['certified']]
    return fewer, cut, tie, cert
