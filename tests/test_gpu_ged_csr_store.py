"""Graph-store GED bounds on the GPU (include/siamese_ged_csr.h) on stores web.CsrStore never
builds but the header permits, and at the limits of the packed (type, degree) word: rows without
their diagonal entry (an isolated node's row is empty), stored zeros, other weights, one-type
graphs near K_300 (degrees up to 298, CSR rows of 300 entries, 16 slots) and types at both ends
of [0, 2^22).  test_ged_csr_store_host.py shows on the host that the variant stores are what
they are called and counts the dense pairs' rounds."""
import time

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _ged_csr_restatement as C
import _ged_csr_store_cases as S
from test_ged_csr_store_host import DENSE_ROUNDS
from test_gpu_ged_csr import LIMIT_512_S, LIMIT_FACTOR, NS_PER_ROUND, _matrix, _plain, _run

pytestmark = pytest.mark.gpu

_SOLVED = {}


def _reference(store, both):
    """The restatement's grid of a whole store; pairs of graphs it has solved already (read
    from another store as the same types and adjacency) are not solved again."""
    ref = C.GridReference(store)
    G = len(store)
    keys = [ref.graph(g)[0].tobytes() + ref.graph(g)[1].tobytes() for g in range(G)]
    for a in range(G):
        for b in range(G):
            if (keys[a], keys[b]) not in _SOLVED:
                _SOLVED[(keys[a], keys[b])] = ref.pair(a, b)
            ref.pairs[(a, b)] = _SOLVED[(keys[a], keys[b])]
    return ref.grid(range(G), range(G), both)


# ---- 1. diagonal, zeros and weights ---------------------------------------------------------
@pytest.mark.parametrize('both', [False, True], ids=['one_order', 'both_orders'])
def test_diagonal_zeros_and_weights_of_the_store_do_not_matter(gpu, both):
    base, var = S.base(), S.variants()
    want = _run(gpu, base, both=both)
    for w, r in zip(want, _reference(base, both)):
        assert np.array_equal(w, r), np.argwhere(w != r)[:5]
    for name in ('nodiag', 'scaled', 'zeros_added'):
        got = _run(gpu, var[name], both=both)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
        for g, r in zip(got, _reference(var[name], both)):
            assert np.array_equal(g, r), (name, np.argwhere(g != r)[:5])
    got = _run(gpu, var['zeros_for_edges'], both=both)
    removed = _run(gpu, var['edges_removed'], both=both)
    for g, w, r in zip(got, removed, _reference(var['zeros_for_edges'], both)):
        assert np.array_equal(g, w), np.argwhere(g != w)[:5]
        assert np.array_equal(g, r), np.argwhere(g != r)[:5]
    assert not np.array_equal(got[0], want[0])       # the zeroed edges did count before


# ---- 2. degree and bisection limits at 16 slots ---------------------------------------------
@pytest.mark.parametrize('a,b', sorted(DENSE_ROUNDS), ids=['K300-pm:K290', 'K257-e:K300-pm'])
def test_dense_pairs_against_scipy(gpu, a, b):
    """K_300 minus a perfect matching against K_290 (174,300 + 174,300 rounds in the numpy
    solver) and K_257 minus an edge against K_300 minus a perfect matching (66,863 + 66,863),
    checked as test_gpu_ged_csr.test_large_pairs_against_scipy checks its pairs.  Time limit:
    rounds x NS_PER_ROUND x LIMIT_FACTOR of that module, 4.18 s and 1.60 s, both below its
    LIMIT_512_S.  Measured on an MI355X: 0.38 s and 0.15 s for the calls."""
    store = S.dense_store()
    limit = sum(DENSE_ROUNDS[(a, b)]) * NS_PER_ROUND * 1e-9 * LIMIT_FACTOR
    assert limit < LIMIT_512_S
    t0 = time.perf_counter()
    ub, lb, mp = _run(gpu, store, [a], [b], both=False)      # returns host arrays: synchronised
    took = time.perf_counter() - t0
    print('call took', took, 's; limit', limit)
    assert took < limit
    n1, n2 = int(store.n[a]), int(store.n[b])
    g1, g2 = _plain(store, a), _plain(store, b)
    (t1, d1, E1), (t2, d2, E2) = g1, g2
    assert max(d1 + d2) >= 289 and mp.shape == (1, 1, S.DENSE_N_MAX)
    phi = [int(x) for x in mp[0, 0, :n1]]
    kept = [x for x in phi if x >= 0]
    assert len(set(kept)) == len(kept) and all(x < n2 for x in kept)
    assert (mp[0, 0, n1:] == -1).all()
    M = _matrix(g1, g2, 1)
    r, c = linear_sum_assignment(M)
    cost = sum(M[i, phi[i]] if phi[i] >= 0 else M[i, n2 + i] for i in range(n1))
    cost += sum(M[n1 + j, j] for j in set(range(n2)) - set(kept))
    print('w=1 assignment cost', cost, 'scipy', M[r, c].sum())
    assert cost == M[r, c].sum()
    subs = sum(1 for i in range(n1) if phi[i] >= 0 and t1[i] != t2[phi[i]])
    both_e = sum(1 for (x, y) in E1 if phi[x] >= 0 and phi[y] >= 0 and (phi[x], phi[y]) in E2)
    induced = (n1 - len(kept)) + (n2 - len(kept)) + subs + (len(E1) + len(E2)) // 2 - both_e
    print('induced', induced, 'ub', int(ub[0, 0]))
    assert induced == ub[0, 0]
    M2 = _matrix(g1, g2, 2)
    r, c = linear_sum_assignment(M2)
    print('lb', int(lb[0, 0]), 'scipy', -(-int(M2[r, c].sum()) // 2))
    assert lb[0, 0] == -(-int(M2[r, c].sum()) // 2)


# ---- 3. types at the ends of [0, 2^22) ------------------------------------------------------
def test_the_largest_types_are_served(gpu):
    """2^22 - 1 fills the packed word up to bit 31; 2^21 - 1 differs from it in bit 21 only.
    The results are those of the same store with the two types renamed to small fresh ones."""
    base = S.base()
    fresh = int(base.types.max()) + 1
    hi, lo = S.MAX_TYPE, S.MAX_TYPE ^ (1 << 21)
    where = ((2, 0), (2, 1), (3, 2), (4, 3), (4, 64))
    names = (hi, lo, hi, lo, hi)
    big = S.retyped(base, [(g, a, t) for (g, a), t in zip(where, names)])
    small = S.retyped(base, [(g, a, fresh + (t == lo)) for (g, a), t in zip(where, names)])
    assert int(big.types.max()) == hi and int(small.types.max()) == fresh + 1
    got = _run(gpu, big, both=True)
    want = _run(gpu, small, both=True)
    plain = _run(gpu, base, both=True)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), np.argwhere(g != w)[:5]
    assert not np.array_equal(got[0], plain[0])      # the new types cost something
    for g, r in zip(got, _reference(big, True)):
        assert np.array_equal(g, r), np.argwhere(g != r)[:5]


@pytest.mark.parametrize('bad', [1 << 22, -1], ids=['2^22', 'minus_one'])
def test_a_type_outside_the_range_is_refused(gpu, bad):
    from graphembedding_amd import _lib
    from graphembedding_amd.ged import ged_grid
    base = S.base()
    G = len(base)
    holed = S.retyped(base, [(1, 4, bad)])
    want = _run(gpu, base, both=True)
    ub, lb, mp, status = _run(gpu, holed, both=True, return_status=True)
    assert int(status[0]) == _lib.SG_ERR_SHAPE
    rest = [g for g in range(G) if g != 1]
    for out in (ub, lb, mp):
        assert (out[1] == -1).all() and (out[:, 1] == -1).all()
    for out, w in zip((ub, lb, mp), want):
        assert np.array_equal(out[np.ix_(rest, rest)], w[np.ix_(rest, rest)])
    with pytest.raises(_lib.SiameseHipError, match='SG_ERR_SHAPE'):
        ged_grid(holed, [1], [0], device=gpu)
    assert int(_run(gpu, holed, [0, 2], [3], return_status=True)[3][0]) == 0
