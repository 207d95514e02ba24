"""The yardstick of the k-nearest GED query (tests/_ged_knn_restatement.py) against brute force
over the exact restatement's matrix and against its own contract, on the host: a certified row
is the true top-k in ascending (distance, column), the sets the GPU test expects certified are
certified, the 16-node search limit withholds the certificate, knn24 shows every branch of the
verify step, and the filter only removes work."""
import numpy as np
import pytest

import _ged_knn_cases as KC
import _ged_knn_restatement as K
from graphembedding_amd import _lib

B = KC.PROVE_BUDGET
# the restatement restates this library's call: without it there is nothing to be a yardstick of
assert K.MAX_K == _lib.GED_KNN_MAX_K


def _ks(name):
    G = len(KC.store(name)[0])
    return sorted({1, 2, 3, G, 64} | ({G + 1} if G == 4 else set()))


CASES = [(name, k) for name in KC.SETS for k in _ks(name)]
_EXACT = {}


def _exact(name):
    """(ub, lb) of ExactGridReference over all pairs of a set at PROVE_BUDGET."""
    if name not in _EXACT:
        store, ref = KC.store(name)
        G = len(store)
        _EXACT[name] = ref.exact.grid(range(G), range(G), B)[:2]
    return _EXACT[name]


def test_the_case_list_is_the_one_asked_for():
    assert len(KC.store('tie10')[0]) == 4 and ('tie10', 5) in CASES
    assert len(KC.store('knn24')[0]) == 24 and KC.store('knn24')[0].n_max == 10
    n = KC.store('knn24')[0].n
    assert n.min() >= 3 and n.max() <= 9


@pytest.mark.parametrize('name,k', CASES, ids=['{}-k{}'.format(*c) for c in CASES])
def test_certified_rows_are_the_true_top_k(name, k):
    store, ref = KC.store(name)
    G = len(store)
    rows = ref.rows(range(G), range(G), k, B)
    eub, elb = _exact(name)
    kq = min(k, G)
    n_brute = 0
    for i, r in enumerate(rows):
        assert len(r['cols']) == k and r['cols'][kq:] == [-1] * (k - kq)
        assert r['ub'][kq:] == [-1] * (k - kq) and r['lb'][kq:] == [-1] * (k - kq)
        assert all(0 <= lo <= up for lo, up in zip(r['lb'][:kq], r['ub'][:kq]))
        if name != 'cap32':
            assert r['certified'] == 1, (i, r)
        if not r['certified']:
            continue
        assert r['ub'][:kq] == r['lb'][:kq]
        if (eub[i] == elb[i]).all():           # the whole row is proven: brute force
            assert r['cols'] == K.brute_force_topk(list(eub[i]), k), i
            assert r['ub'][:kq] == [int(eub[i, j]) for j in r['cols'][:kq]]
            n_brute += 1
            continue
        # some distance of the row is known by its bounds only (cap32): what must hold of
        # them if the row is the true top-k
        sel = r['cols'][:kq]
        d, s = r['ub'][kq - 1], sel[-1]
        for j, u in zip(sel, r['ub']):
            assert elb[i, j] <= u <= eub[i, j], (i, j)
        for j in range(G):
            if j not in sel:
                assert eub[i, j] > d or (eub[i, j] == d and j > s), (i, j)
    assert n_brute == G or name == 'cap32'


def test_knn24_shows_every_branch_at_k_3():
    store, ref = KC.store('knn24')
    G = len(store)
    fewer, cut, tie, cert = KC.knn24_properties(ref, 3, B)
    assert fewer, '(a) no row with fewer candidates than columns'
    assert cut, '(b) no pair proven out by the cutoff'
    assert tie, '(c) no tie in ub at the k-th place'
    assert len(cert) == G, '(d) rows left uncertified'
    rows = ref.rows(range(G), range(G), 3, B)
    i, j = cut[0]
    ub0, lb0, c, u, l, e = rows[i]['pairs'][j]
    assert lb0 <= rows[i]['tau'] < c < ub0 and (u, l) == (ub0, c) and e > 0
    # (c): the tied pair left out is proven at the same distance, so only the column decides
    r = rows[tie[0]]
    out = [jj for jj, p in r['pairs'].items() if p[3] == r['ub'][2] and jj > r['cols'][2]]
    assert out and all(jj not in r['cols'] for jj in out)


def test_the_filter_only_removes_work():
    store, ref = KC.store('knn24')
    G = len(store)
    spent = sum(r['expansions'] for r in ref.rows(range(G), range(G), 3, B))
    whole = int(ref.exact.grid(range(G), range(G), B)[3].sum())
    listed = sum(r['candidates'] for r in ref.rows(range(G), range(G), 3, B))
    print('knn24 k=3: {} of {} pairs are candidates, {} of {} expansions'.format(
        listed, G * G, spent, whole))
    assert 0 < spent <= whole and listed < G * G


def test_cap32_certificates_stop_at_the_search_limit():
    store, ref = KC.store('cap32')
    G = len(store)
    n = store.n
    hinged, by_bounds = 0, 0
    for k in _ks('cap32'):
        for i, r in enumerate(ref.rows(range(G), range(G), k, B)):
            kq = min(k, G)
            sel = r['cols'][:kq]
            d = r['ub'][kq - 1]
            big = [j for j, p in r['pairs'].items()
                   if max(n[i], n[j]) > K.X.MAX_SEARCH_NODES and p[3] != p[4]
                   and (j in sel or p[4] < d)]
            if big:                            # the answer hinges on a pair nobody searched
                assert r['certified'] == 0, (k, i)
                assert all(r['pairs'][j][5] == 0 for j in big)
                hinged += 1
            if r['certified'] and r['expansions'] == 0:
                by_bounds += 1
    assert hinged and by_bounds


def test_unservable_entries_and_short_databases():
    import copy
    store, _ = KC.store('cap10')
    holed = copy.copy(store)
    holed.n = store.n.copy()
    holed.n[4] = 0
    ref = K.KnnReference(holed)
    G = len(store)
    cols, ub, lb, cert, cand, ex = ref.knn([3, -1, 4, G, 6], [9, 4, 3, 2 ** 31 - 1, 7], 4, 7)
    assert (cols[[1, 2, 3]] == -1).all() and (ub[[1, 2, 3]] == -1).all()
    assert (lb[[1, 2, 3]] == -1).all() and not cert[[1, 2, 3]].any()
    assert (cand[[1, 2, 3]] == -1).all() and (ex[[1, 2, 3]] == -1).all()
    for i in (0, 4):                           # three servable columns: k' = 3
        assert set(cols[i, :3]) == {0, 2, 4} and cols[i, 3] == -1 and ub[i, 3] == lb[i, 3] == -1
    full = ref.knn([3, 6], [9, 3, 7], 3, 7)    # the same rows without the holes
    assert np.array_equal(cols[[0, 4], :3] // 2, full[0])      # columns 0, 2, 4 are 0, 1, 2 there
    assert np.array_equal(ub[[0, 4], :3], full[1]) and np.array_equal(lb[[0, 4], :3], full[2])
    none = ref.knn([3], [4, -1], 2, 7)         # no servable column: nothing to find
    assert (none[0] == -1).all() and none[3][0] == 1 and none[4][0] == 0 and none[5][0] == 0


def test_knn_recall_counts_certified_rows_only():
    from graphembedding_amd.ged import knn_recall
    true = np.array([[0, 1, 2], [3, 4, -1], [5, 6, 7], [-1, -1, -1]])
    pred = np.array([[2, 9, 0, 8], [4, 3, 1, 0], [0, 0, 0, 0], [1, 2, 3, 4]])
    r, rows = knn_recall(pred, true, [1, 1, 0, 1])
    assert rows == 2 and r == pytest.approx((2 / 3 + 2 / 2) / 2)
    r, rows = knn_recall(pred, true, [0, 0, 0, 0])
    assert rows == 0 and np.isnan(r)
    assert knn_recall(true, true, [1, 1, 1, 1]) == (1.0, 3)
    with pytest.raises(ValueError):
        knn_recall(pred[:2], true, [1, 1, 1, 1])
