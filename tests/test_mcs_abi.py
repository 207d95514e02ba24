"""Host side of the budgeted MCS search (include/siamese_mcs.h): the library exports the
header's symbols, the unit is a source of the library, the workspace query follows
sg_ged_grid's, and every refusal of sg_mcs_grid comes in the header's order before any HIP call
(dummy pointers, so all of this runs without a GPU)."""
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


def test_mcs_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_mcs.h')
    assert syms == sorted(['sg_mcs_grid_workspace_bytes', 'sg_mcs_grid'])
    assert set(syms) == set(_lib.MCS_SYMBOLS)
    for s in syms:
        assert hasattr(L, s), s
    for fn in ('mcs_grid_workspace_bytes', 'mcs_grid'):
        assert callable(getattr(_lib, fn)), fn
    assert L.sg_version() == 11000
    assert "symbols' presence" in open(os.path.join(ROOT, 'include', 'siamese_mcs.h')).read()
    # the GED headers keep their own
    assert set(_header_symbols('siamese_ged.h')) == set(_lib.GED_SYMBOLS)
    assert set(_header_symbols('siamese_ged_exact.h')) == set(_lib.GED_EXACT_SYMBOLS)
    for other in (_lib.GED_SYMBOLS, _lib.GED_EXACT_SYMBOLS, _lib.GED_BEAM_SYMBOLS,
                  _lib.GED_CSR_SYMBOLS):
        assert not set(other) & set(_lib.MCS_SYMBOLS)


def test_mcs_unit_is_a_source_of_the_library():
    from graphembedding_amd import build
    assert 'sg_mcs.hip' in build.SOURCES and 'sg_ged.hip' in build.SOURCES
    assert 'sg_ged_common.h' in build.HEADERS
    for f in ('sg_mcs.hip', 'sg_ged_common.h'):
        assert os.path.isfile(os.path.join(build.CSRC, f))
    # the prep kernel and the workspace entry are shared, not copied
    src = open(os.path.join(build.CSRC, 'sg_mcs.hip')).read()
    assert '#include "sg_ged_common.h"' in src and 'ged_launch_prep(' in src
    assert 'sg_ged_prep_kernel' not in src


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _rc(L, m=3, n=5, ld=None, n_graphs=8, n_max=10, connected=0, budget=100, **null):
    """sg_mcs_grid with dummy non-null pointers (name=0 passes NULL): only paths that return
    before the first launch are exercised."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_mcs_grid(p('adj'), p('types'), p('sn'), n_graphs, n_max, p('q'), m, p('db'), n,
                         connected, budget, p('size'), n if ld is None else ld, p('bound'),
                         p('edges'), p('map'), p('exp'), p('status'), p('ws'), None)


def test_mcs_argument_rules(L):
    """The header's table, rule by rule and in its order: a later rule's violation never hides
    an earlier one's.  `adj=0` (the last rule) marks calls that pass every other rule."""
    ws = L.sg_mcs_grid_workspace_bytes
    top = 1 << 24
    # 1. negative sizes, before anything else
    assert _rc(L, m=-1) == A and ws(-1, 5, 10) == -1
    assert _rc(L, n=-1) == A and ws(3, -1, 10) == -1
    assert _rc(L, ld=-1) == A
    assert _rc(L, m=-1, n_max=33) == A
    assert _rc(L, ld=-1, budget=top + 1) == A
    # 2. n_graphs < 0, n_max < 1
    assert _rc(L, n_graphs=-1) == A
    assert _rc(L, n_graphs=-1, n_max=33) == A
    assert _rc(L, n_max=0) == A and ws(3, 5, 0) == -1
    assert _rc(L, n_max=-4, budget=top + 1) == A and ws(3, 5, -4) == -1
    assert _rc(L, n_graphs=0, adj=0) == A                # an empty store passes on (all ids bad)
    # 3. n_max > 32
    assert _rc(L, n_max=33) == U and ws(3, 5, 33) == -1
    assert _rc(L, n_max=33, ld=2) == U                   # before ld < n
    assert _rc(L, n_max=33, connected=2) == U            # before connected
    assert _rc(L, n_max=33, budget=-1) == U              # before the budget
    assert _rc(L, n_max=33, m=0) == U                    # before the empty call
    assert _rc(L, n_max=32, adj=0) == A and ws(3, 5, 32) == 4 * 8 * 68
    assert _rc(L, n_max=1, adj=0) == A and ws(3, 5, 1) == 4 * 8 * 4
    # 4. grid sizes
    big = top + 1
    assert _rc(L, m=big) == U and ws(big, 5, 10) == -1
    assert _rc(L, n=big, ld=big) == U and ws(3, big, 10) == -1
    assert _rc(L, m=top, n=257, ld=257) == U and ws(top, 257, 10) == -1
    assert _rc(L, m=top, n=256, ld=256, adj=0) == A
    assert _rc(L, m=big, ld=2) == U                      # before ld < n
    assert _rc(L, m=big, connected=-1) == U              # before connected
    assert _rc(L, m=big, budget=-1) == U                 # before the budget
    # 5. ld < n
    assert _rc(L, ld=4) == A
    assert _rc(L, ld=4, budget=top + 1) == A             # before the budget's ceiling
    assert _rc(L, m=0, ld=4) == A                        # before the empty call
    assert _rc(L, ld=9, adj=0) == A                      # ld > n is fine: on to the pointers
    # 6. connected outside {0, 1}, next to the budget rules and before them
    assert _rc(L, connected=2) == A
    assert _rc(L, connected=-1) == A
    assert _rc(L, connected=2, budget=top + 1) == A      # before the budget's ceiling
    assert _rc(L, connected=2, m=0) == A                 # before the empty call
    assert _rc(L, connected=1, adj=0) == A               # 1 passes on
    # 7. max_expansions < 0
    assert _rc(L, budget=-1) == A
    assert _rc(L, budget=-(1 << 40)) == A
    assert _rc(L, m=0, budget=-1) == A                   # before the empty call
    # 8. max_expansions > 2^24
    assert _rc(L, budget=top + 1) == U
    assert _rc(L, budget=1 << 40) == U
    assert _rc(L, n=0, ld=0, budget=top + 1) == U        # before the empty call
    assert _rc(L, budget=top + 1, adj=0) == U            # before the pointers
    assert _rc(L, budget=top, adj=0) == A                # 2^24 itself and 0 pass on
    assert _rc(L, budget=0, adj=0) == A
    # 9. empty grids: no work, whatever the pointers
    assert _rc(L, m=0, adj=0, types=0, sn=0, size=0, bound=0, ws=0) == OK
    assert _rc(L, n=0, ld=0, adj=0, types=0, sn=0, size=0, bound=0, ws=0) == OK
    assert ws(0, 5, 10) == 0 and ws(3, 0, 10) == 0
    # 10. the required pointers (bound_out among them); q_idx, db_idx, edges_out, map_out,
    # expansions_out and status_out may be NULL
    for null in ('adj', 'types', 'sn', 'size', 'bound', 'ws'):
        assert _rc(L, **{null: 0}) == A, null
    assert _rc(L, q=0, db=0, edges=0, map=0, exp=0, status=0, adj=0) == A


def test_mcs_workspace_is_the_bipartite_call_s(L):
    ws, ws0 = L.sg_mcs_grid_workspace_bytes, L.sg_ged_grid_workspace_bytes
    for shape in [(3, 5, 10), (700, 700, 10), (1, 1, 1), (6, 6, 32), (1 << 24, 256, 10),
                  (0, 5, 10), (3, 5, 33), (-1, 5, 10), ((1 << 24) + 1, 1, 10)]:
        assert ws(*shape) == ws0(*shape), shape
    assert ws(3, 5, 10) == 4 * 8 * 24
    with pytest.raises(_lib.SiameseHipError, match='sg_mcs_grid_workspace_bytes'):
        _lib.mcs_grid_workspace_bytes(3, 5, 33)
    assert _lib.mcs_grid_workspace_bytes(3, 5, 10) == 768
    assert _lib.MCS_MAX_BUDGET == 1 << 24


def test_python_layer_defaults_and_the_untouched_ged():
    import inspect

    from graphembedding_amd import distance, mcs
    assert mcs.MCS_DEFAULT_BUDGET == 1 << 20 <= _lib.MCS_MAX_BUDGET
    sig = inspect.signature(mcs.mcs_grid).parameters
    assert sig['connected'].default is False and sig['budget'].default == mcs.MCS_DEFAULT_BUDGET
    for opt in ('bounds', 'edges', 'mapping', 'expansions', 'return_status'):
        assert sig[opt].default is False, opt
    assert inspect.signature(distance.mcs).parameters['connected'].default is False
    doc = ' '.join(distance.mcs.__doc__.split())
    assert 'node count of a maximum common induced subgraph' in doc and 'type equality' in doc
    assert 'not chorus' in doc and 'not claimed' in doc
    with pytest.raises(RuntimeError, match='graph-matching-toolkit'):
        distance.ged(None, None, 'astar')                # distance.ged is untouched
