"""What test_gpu_ged_csr_store.py relies on, without a GPU: the variant stores of
_ged_csr_store_cases.py are what they are called and keep the preconditions of
include/siamese_ged_csr.h (columns strictly ascending, the pattern symmetric), the restatement
(tests/_ged_csr_restatement.py) reads each of them as the graph it stands for, the types at the
end of the range fill the packed word, and the dense pair's round count gives a time limit below
the (512, 512) pair's."""
import numpy as np

import _ged_csr_restatement as C
import _ged_csr_store_cases as S

# rounds of the numpy solver (w = 1, w = 2) on K_300 - pm against K_290 and on K_257 - e against
# K_300 - pm, counted again by test_the_dense_pairs_stay_below_the_512_pair (about 15 s)
DENSE_ROUNDS = {(0, 1): (174300, 174300), (2, 0): (66863, 66863)}
ROUNDS_512 = 409538 + 405737          # test_gpu_ged_csr.py's, whose limit the dense pair keeps


def _rows(store):
    for g in range(len(store)):
        off, n = int(store.node_off[g]), int(store.n[g])
        for a in range(n):
            s0, s1 = int(store.row_ptr[off + a]), int(store.row_ptr[off + a + 1])
            yield g, a, n, store.col[s0:s1], store.val[s0:s1]


def test_the_variants_are_what_they_are_called():
    base, var = S.base(), S.variants()
    assert base.n.tolist() == list(S.SIZES) + [sum(S.ISOLATED)]
    for store in [base] + list(var.values()):
        assert int(store.row_ptr[-1]) == store.col.size == store.val.size
        for g, a, n, cols, vals in _rows(store):
            assert (np.diff(cols) > 0).all() and (cols >= 0).all() and (cols < n).all()
        for g in range(len(store)):
            P, V = S.dense_of(store, g)
            assert np.array_equal(P, P.T) and np.array_equal(V, V.T)
    # the store web.CsrStore builds: every row holds its diagonal entry, no stored zero, and
    # weights that are not 1 already
    for g, a, n, cols, vals in _rows(base):
        assert a in cols and (vals != 0).all()
    assert ((base.val != 1) & (base.val != 0)).any()
    rows = {k: list(_rows(s)) for k, s in var.items()}
    assert all(a not in cols for g, a, n, cols, vals in rows['nodiag'])
    empty = [(g, a) for g, a, n, cols, vals in rows['nodiag'] if cols.size == 0]
    assert empty == [(0, 0)] + [(len(S.SIZES), a) for a in range(S.ISOLATED[0], sum(S.ISOLATED))]
    assert np.array_equal(var['scaled'].col, base.col)
    assert np.array_equal(var['scaled'].val, base.val * np.float32(S.WEIGHT))
    extra = var['zeros_added'].col.size - base.col.size
    assert extra > 0 and extra == int((var['zeros_added'].val == 0).sum())
    assert all(a not in cols[vals == 0] for g, a, n, cols, vals in rows['zeros_added'])
    gone = S.zeroed_edges()
    assert np.array_equal(var['zeros_for_edges'].col, base.col)
    assert int((var['zeros_for_edges'].val == 0).sum()) == 2 * sum(len(x) for x in gone) > 0
    assert not (var['edges_removed'].val == 0).any()
    assert [len(x) for x in gone][0] == 0 and all(len(x) > 0 for x in gone[1:])


def test_the_restatement_reads_every_variant():
    """(a) to (c) stand for the base store's graphs, (d) for the graphs without its edges."""
    base, var = S.base(), S.variants()
    n_changed = 0
    for g in range(len(base)):
        t, A = C.graph_of_store(base, g)
        for name in ('nodiag', 'scaled', 'zeros_added'):
            vt, vA = C.graph_of_store(var[name], g)
            assert np.array_equal(vt, t) and np.array_equal(vA, A), (name, g)
        zt, zA = C.graph_of_store(var['zeros_for_edges'], g)
        rt, rA = C.graph_of_store(var['edges_removed'], g)
        assert np.array_equal(zt, rt) and np.array_equal(zA, rA) and np.array_equal(zt, t)
        assert int(A.sum()) - int(zA.sum()) == 2 * len(S.zeroed_edges()[g])
        n_changed += not np.array_equal(zA, A)
    assert n_changed == len(base) - 1


def test_type_limits_fill_the_packed_word():
    assert S.MAX_TYPE == (1 << 22) - 1
    assert ((S.MAX_TYPE << 10) | 1023) == (1 << 32) - 1              # bit 31 of the word
    assert S.MAX_TYPE ^ (1 << 21) == (1 << 21) - 1                   # differs in bit 21 only
    assert int(S.base().types.max()) < 8                             # fresh small names exist


def test_the_dense_set_reaches_the_degree_and_bisection_limits():
    store = S.dense_store()
    assert store.n_max == S.DENSE_N_MAX and (2 * store.n_max + 63) // 64 > 8      # 16 slots
    assert store.n.tolist() == [300, 290, 257] and len(set(store.types.tolist())) == 1
    deg = []
    for g, a, n, cols, vals in _rows(store):
        assert a in cols and cols.size >= 256                         # 2^8 entries or more
        deg.append(cols.size - 1)
    assert max(deg) == 298 and deg[300] == 289 and min(deg[590:]) == 255
    # 300 entries a row and 300 rows: both bisections need nine of their ten steps
    assert 1 << 8 < int(np.diff(store.row_ptr).max()) == 299 < 1 << 9


def test_the_dense_pairs_stay_below_the_512_pair():
    store = S.dense_store()
    for (a, b), want in DENSE_ROUNDS.items():
        g1, g2 = C.graph_of_store(store, a), C.graph_of_store(store, b)
        rounds = []
        for w in (1, 2):
            count = [0]
            C.lsap(C.cost_matrix(g1, g2, w), count)
            rounds.append(count[0])
        print((a, b), 'rounds', rounds)
        assert tuple(rounds) == want and sum(rounds) < ROUNDS_512
