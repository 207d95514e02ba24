"""Host side of the k-nearest GED query (include/siamese_ged_knn.h): the library exports the
header's symbols next to the unchanged bipartite and exact sets, the workspace query is the
documented formula, and every refusal of sg_ged_knn comes in the header's order before any HIP
call (dummy pointers, so all of this runs without a GPU).  The Python layer's signature and
raises that need no device."""
import ctypes
import os
import re

import pytest

from graphembedding_amd import _lib
from graphembedding_amd.build import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM_RE = r'^\s*(?:int32_t|int64_t)\s+(sg_\w+)\s*\('   # test_lib_abi.header_symbols
A, U, OK = _lib.SG_ERR_ARG, _lib.SG_ERR_UNSUPPORTED, _lib.SG_OK


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def test_knn_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_ged_knn.h')
    assert syms == sorted(['sg_ged_knn_workspace_bytes', 'sg_ged_knn'])
    assert set(syms) == set(_lib.GED_KNN_SYMBOLS)
    for s in syms:
        assert hasattr(L, s), s
    for fn in ('ged_knn_workspace_bytes', 'ged_knn'):
        assert callable(getattr(_lib, fn)), fn
    assert L.sg_version() == 11000
    assert "symbols' presence" in open(os.path.join(ROOT, 'include',
                                                    'siamese_ged_knn.h')).read()
    # the bipartite and exact headers keep their own
    assert set(_header_symbols('siamese_ged.h')) == set(_lib.GED_SYMBOLS)
    assert set(_header_symbols('siamese_ged_exact.h')) == set(_lib.GED_EXACT_SYMBOLS)
    assert not set(_lib.GED_KNN_SYMBOLS) & (set(_lib.GED_SYMBOLS) | set(_lib.GED_EXACT_SYMBOLS))


def test_knn_unit_is_a_source_of_the_library():
    from graphembedding_amd import build
    assert 'sg_ged_knn.hip' in build.SOURCES and 'sg_ged_exact.hip' in build.SOURCES
    assert 'sg_ged_search.h' in build.HEADERS and 'sg_ged_common.h' in build.HEADERS
    for f in ('sg_ged_knn.hip', 'sg_ged_search.h'):
        assert os.path.isfile(os.path.join(build.CSRC, f))
    # both units take the search from the shared header
    for f in ('sg_ged_knn.hip', 'sg_ged_exact.hip'):
        assert '#include "sg_ged_search.h"' in open(os.path.join(build.CSRC, f)).read()


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _rc(L, m=3, n=5, n_graphs=8, n_max=10, k=3, budget=100, **null):
    """sg_ged_knn with dummy non-null pointers (name=0 passes NULL): only paths that return
    before the first HIP call are exercised."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_ged_knn(p('adj'), p('types'), p('sn'), n_graphs, n_max, p('q'), m, p('db'), n,
                        k, budget, p('col'), p('ub'), p('lb'), p('cert'), p('cand'), p('exp'),
                        p('status'), p('ws'), None)


def test_knn_argument_rules(L):
    """The header's table, rule by rule and in its order: a later rule's violation never hides
    an earlier one's.  `adj=0` (the last rule) marks calls that pass every other rule."""
    ws = L.sg_ged_knn_workspace_bytes
    top = 1 << 24
    # 1. negative sizes, before anything else
    assert _rc(L, m=-1) == A and ws(-1, 5, 10, 3) == -1
    assert _rc(L, n=-1) == A and ws(3, -1, 10, 3) == -1
    assert _rc(L, m=-1, n_max=33) == A
    assert _rc(L, n=-1, k=65) == A
    # 2. n_graphs < 0, n_max < 1
    assert _rc(L, n_graphs=-1) == A
    assert _rc(L, n_graphs=-1, n_max=33) == A
    assert _rc(L, n_max=0) == A and ws(3, 5, 0, 3) == -1
    assert _rc(L, n_max=-4, k=65) == A
    assert _rc(L, n_graphs=0, adj=0) == A                # an empty store passes on (all ids bad)
    # 3. n_max > 32
    assert _rc(L, n_max=33) == U and ws(3, 5, 33, 3) == -1
    assert _rc(L, n_max=33, k=0) == U                    # before k
    assert _rc(L, n_max=33, budget=-1) == U              # before the budget
    assert _rc(L, n_max=33, m=0) == U                    # before the empty call
    assert _rc(L, n_max=32, adj=0) == A
    # 4. grid sizes
    big = top + 1
    assert _rc(L, m=big) == U and ws(big, 5, 10, 3) == -1
    assert _rc(L, n=big) == U and ws(3, big, 10, 3) == -1
    assert _rc(L, m=top, n=257) == U and ws(top, 257, 10, 3) == -1
    assert _rc(L, m=top, n=256, adj=0) == A
    assert _rc(L, m=big, k=0) == U                       # before k
    assert _rc(L, m=big, budget=-1) == U                 # before the budget
    # 5. k < 1
    assert _rc(L, k=0) == A and ws(3, 5, 10, 0) == -1
    assert _rc(L, k=-7) == A and ws(3, 5, 10, -7) == -1
    assert _rc(L, k=0, budget=top + 1) == A              # before the budget's ceiling
    assert _rc(L, k=0, m=0) == A                         # before the empty call
    # 6. k > 64
    assert _rc(L, k=65) == U and ws(3, 5, 10, 65) == -1
    assert _rc(L, k=65, budget=-1) == U                  # before the budget
    assert _rc(L, k=65, n=0) == U                        # before the empty call
    assert _rc(L, k=64, adj=0) == A and _rc(L, k=1, adj=0) == A
    assert _rc(L, k=64, n=2, adj=0) == A                 # k above n is fine
    # 7. max_expansions < 0
    assert _rc(L, budget=-1) == A
    assert _rc(L, budget=-(1 << 40)) == A
    assert _rc(L, m=0, budget=-1) == A                   # before the empty call
    # 8. max_expansions > 2^24
    assert _rc(L, budget=top + 1) == U
    assert _rc(L, budget=1 << 40) == U
    assert _rc(L, n=0, budget=top + 1) == U              # before the empty call
    assert _rc(L, budget=top + 1, adj=0) == U            # before the pointers
    assert _rc(L, budget=top, adj=0) == A                # 2^24 itself and 0 pass on
    assert _rc(L, budget=0, adj=0) == A
    # 9. empty grids: no work, whatever the pointers
    every = dict(adj=0, types=0, sn=0, col=0, ub=0, lb=0, cert=0, ws=0)
    assert _rc(L, m=0, **every) == OK
    assert _rc(L, n=0, **every) == OK
    assert ws(0, 5, 10, 3) == 0 and ws(3, 0, 10, 3) == 0
    # 10. the required pointers; q_idx, db_idx, candidates_out, expansions_out and status_out
    # may be NULL
    for null in ('adj', 'types', 'sn', 'col', 'ub', 'lb', 'cert', 'ws'):
        assert _rc(L, **{null: 0}) == A, null
    assert _rc(L, q=0, db=0, cand=0, exp=0, status=0, adj=0) == A
    # 11. the workspace's alignment, after the pointers and still before any HIP call
    assert _P % 8 == 0
    for off in (1, 2, 4, 7):
        assert L.sg_ged_knn(_P, _P, _P, 8, 10, _P, 3, _P, 5, 3, 100, _P, _P, _P, _P, _P, _P, _P,
                            _P + off, None) == A, off
    assert L.sg_ged_knn(_P, _P, _P, 8, 10, _P, 3, _P, 5, 3, 100, None, _P, _P, _P, _P, _P, _P,
                        _P + 4, None) == A


def test_knn_workspace_is_the_documented_formula(L):
    ws = L.sg_ged_knn_workspace_bytes
    for m, n, nm, k in [(3, 5, 10, 3), (140, 560, 10, 10), (1, 1, 1, 1), (6, 6, 32, 64),
                        (1, 4096, 10, 3), (1 << 24, 256, 10, 64)]:
        W = (2 * nm + 4) & ~3
        assert ws(m, n, nm, k) == 16 + 4 * ((m + n) * W + 5 * m * n + 2 * m), (m, n, nm, k)
        assert ws(m, n, nm, k) == ws(m, n, nm, 1)        # k sizes nothing
    assert ws(3, 5, 10, 3) == 1108
    assert 'W = (2 * n_max + 4) & ~3' in open(os.path.join(ROOT, 'include',
                                                           'siamese_ged_knn.h')).read()
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_knn_workspace_bytes'):
        _lib.ged_knn_workspace_bytes(3, 5, 10, 65)
    assert _lib.ged_knn_workspace_bytes(3, 5, 10, 3) == 1108
    assert _lib.GED_KNN_MAX_K == 64


def test_python_signature_and_deviceless_raises():
    import inspect

    from graphembedding_amd import ged
    from graphembedding_amd.ged import csr_store_of_graphs
    sig = inspect.signature(ged.ged_knn)
    assert list(sig.parameters) == ['store', 'q_idx', 'db_idx', 'k', 'exact_budget', 'device',
                                    'stats', 'return_status']
    assert sig.parameters['k'].default == 10
    assert sig.parameters['exact_budget'].default == ged.GED_EXACT_DEFAULT_BUDGET
    assert sig.parameters['stats'].default is False
    assert sig.parameters['return_status'].default is False
    assert callable(ged.ged_knn_graphs) and callable(ged.knn_recall)
    import _ged_exact_cases as C
    with pytest.raises(ValueError, match='CSR'):
        ged.ged_knn(csr_store_of_graphs(C.graphs('cap10')), k=3)
    store, _ = C.store('cap10')
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match='k '):
            ged.ged_knn(store, k=bad)
    for bad in (-1, (1 << 24) + 1):
        with pytest.raises(ValueError, match='exact_budget'):
            ged.ged_knn(store, k=3, exact_budget=bad)
    assert 'siamese_ged_knn.h' in ged.__doc__
