"""Host side of the GED refinement (include/siamese_ged_refine.h): the library exports the
header's symbols next to the unchanged sets of the other GED headers, the workspace query
follows sg_ged_grid's, and every refusal of sg_ged_refine_grid comes in the header's order before
any HIP call (dummy pointers, so all of this runs without a GPU).  The Python layer's opt-ins
keep their defaults."""
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


def test_refine_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_ged_refine.h')
    assert syms == sorted(['sg_ged_refine_grid_workspace_bytes', 'sg_ged_refine_grid'])
    assert set(syms) == set(_lib.GED_REFINE_SYMBOLS)
    for s in syms:
        assert hasattr(L, s), s
    for fn in ('ged_refine_grid_workspace_bytes', 'ged_refine_grid'):
        assert callable(getattr(_lib, fn)), fn
    assert L.sg_version() == 11000
    src = open(os.path.join(ROOT, 'include', 'siamese_ged_refine.h')).read()
    assert "symbols' presence" in src
    assert '2 - mismatch + 2 (kept edges at a) >= 1' in src      # why no move deletes alone
    # the sibling headers keep their own two each
    for name, other in (('siamese_ged.h', _lib.GED_SYMBOLS),
                        ('siamese_ged_exact.h', _lib.GED_EXACT_SYMBOLS),
                        ('siamese_ged_beam.h', _lib.GED_BEAM_SYMBOLS),
                        ('siamese_ged_csr.h', _lib.GED_CSR_SYMBOLS)):
        assert set(_header_symbols(name)) == set(other), name
        assert not set(_lib.GED_REFINE_SYMBOLS) & set(other), name


def test_refine_unit_is_a_source_of_the_library():
    from graphembedding_amd import build
    for f in ('sg_ged_refine.hip', 'sg_ged_beam.hip', 'sg_ged.hip'):
        assert f in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, f))
    assert 'sg_ged_common.h' in build.HEADERS
    assert 'siamese_ged_refine.h' in open(build.__file__).read()     # a dependency of the build


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _rc(L, m=3, n=5, ld=None, n_graphs=8, n_max=10, max_moves=7, **null):
    """sg_ged_refine_grid with dummy non-null pointers (name=0 passes NULL): only paths that
    return before the first launch are exercised."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_ged_refine_grid(p('adj'), p('types'), p('sn'), n_graphs, n_max, p('q'), m,
                                p('db'), n, max_moves, p('ub'), n if ld is None else ld,
                                p('lb'), p('map'), p('moves'), p('status'), p('ws'), None)


def test_refine_argument_rules(L):
    """The header's table, rule by rule and in its order: a later rule's violation never hides
    an earlier one's.  `adj=0` (the last rule) marks calls that pass every other rule."""
    ws = L.sg_ged_refine_grid_workspace_bytes
    top = 1 << 24
    # 1. negative sizes, before anything else
    assert _rc(L, m=-1) == A and ws(-1, 5, 10) == -1
    assert _rc(L, n=-1) == A and ws(3, -1, 10) == -1
    assert _rc(L, ld=-1) == A
    assert _rc(L, m=-1, n_max=33) == A
    assert _rc(L, ld=-1, max_moves=4097) == A
    # 2. n_graphs < 0, n_max < 1
    assert _rc(L, n_graphs=-1) == A
    assert _rc(L, n_graphs=-1, n_max=33) == A
    assert _rc(L, n_max=0) == A and ws(3, 5, 0) == -1
    assert _rc(L, n_max=-4, max_moves=4097) == A and ws(3, 5, -4) == -1
    assert _rc(L, n_graphs=0, adj=0) == A                # an empty store passes on (all ids bad)
    # 3. n_max > 32
    assert _rc(L, n_max=33) == U and ws(3, 5, 33) == -1
    assert _rc(L, n_max=33, ld=2) == U                   # before ld < n
    assert _rc(L, n_max=33, max_moves=-1) == U           # before the move limit
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
    assert _rc(L, m=big, max_moves=-1) == U              # before the move limit
    # 5. ld < n
    assert _rc(L, ld=4) == A
    assert _rc(L, ld=4, max_moves=4097) == A             # before the limit's ceiling
    assert _rc(L, m=0, ld=4) == A                        # before the empty call
    assert _rc(L, ld=9, adj=0) == A                      # ld > n is fine: on to the pointers
    # 6. max_moves < 0
    assert _rc(L, max_moves=-1) == A
    assert _rc(L, max_moves=-(1 << 31)) == A
    assert _rc(L, m=0, max_moves=-1) == A                # before the empty call
    # 7. max_moves > 4096
    assert _rc(L, max_moves=4097) == U
    assert _rc(L, max_moves=(1 << 31) - 1) == U
    assert _rc(L, n=0, ld=0, max_moves=4097) == U        # before the empty call
    assert _rc(L, max_moves=4097, adj=0) == U            # before the pointers
    assert _rc(L, max_moves=4096, adj=0) == A            # 4096 itself and 0 pass on
    assert _rc(L, max_moves=0, adj=0) == A
    # 8. empty grids: no work, whatever the pointers
    assert _rc(L, m=0, adj=0, types=0, sn=0, ub=0, lb=0, ws=0) == OK
    assert _rc(L, n=0, ld=0, adj=0, types=0, sn=0, ub=0, lb=0, ws=0) == OK
    assert ws(0, 5, 10) == 0 and ws(3, 0, 10) == 0
    # 9. the required pointers (lb_out among them); q_idx, db_idx, map_out, moves_out and
    # status_out may be NULL
    for null in ('adj', 'types', 'sn', 'ub', 'lb', 'ws'):
        assert _rc(L, **{null: 0}) == A, null
    assert _rc(L, q=0, db=0, map=0, moves=0, status=0, adj=0) == A


def test_refine_workspace_is_the_bipartite_call_s(L):
    ws, ws0 = L.sg_ged_refine_grid_workspace_bytes, L.sg_ged_grid_workspace_bytes
    for shape in [(3, 5, 10), (700, 700, 10), (1, 1, 1), (6, 6, 32), (1 << 24, 256, 10),
                  (0, 5, 10), (3, 5, 33), (-1, 5, 10), ((1 << 24) + 1, 1, 10)]:
        assert ws(*shape) == ws0(*shape), shape
    assert ws(3, 5, 10) == 4 * 8 * 24
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_refine_grid_workspace_bytes'):
        _lib.ged_refine_grid_workspace_bytes(3, 5, 33)
    assert _lib.ged_refine_grid_workspace_bytes(3, 5, 10) == 768
    assert _lib.GED_REFINE_MAX_MOVES == 4096


def test_python_opt_ins_keep_their_defaults():
    import inspect

    from graphembedding_amd import allpairs, ged
    from graphembedding_amd.config import Flags
    assert Flags().ged_labels == 'synthetic'
    for fn in (ged.ged_grid, ged.ged_matrix, ged.ged_pair):
        assert inspect.signature(fn).parameters['refine_moves'].default is None
    assert inspect.signature(ged.ged_grid).parameters['moves'].default is False
    assert ged.GED_REFINE_DEFAULT_MOVES == 1024 <= _lib.GED_REFINE_MAX_MOVES
    assert inspect.signature(ged.refine_label_matrix).parameters['moves'].default == 1024
    with pytest.raises(RuntimeError, match='with_store=True'):
        allpairs.load_graph_set('syn_aids80nef', ged='bpswap', with_store=False)
    for bad in ('bpswap2', 'swap', 'krefine'):
        with pytest.raises(RuntimeError, match='Unknown ged labels'):
            allpairs.load_graph_set('syn_aids80nef', ged=bad)


def test_ged_grid_refuses_before_it_touches_a_device():
    """The keyword rules of ged_grid come before the store is moved to the device."""
    from graphembedding_amd import ged

    class Store(object):          # to_device would need a GPU: the rules must not reach it
        n_max = 10

        def to_device(self, device):
            raise AssertionError('reached the device')

    with pytest.raises(ValueError, match='mutually exclusive'):
        ged.ged_grid(Store(), refine_moves=7, beam_width=7)
    with pytest.raises(ValueError, match='mutually exclusive'):
        ged.ged_grid(Store(), refine_moves=7, exact_budget=7)
    with pytest.raises(ValueError, match='refine_moves'):
        ged.ged_grid(Store(), moves=True)
    with pytest.raises(ValueError, match='both assignment orders'):
        ged.ged_grid(Store(), refine_moves=7, both_orders=False)


def test_distance_ged_names_the_refinement_bpswap():
    from graphembedding_amd import distance
    for algo in ('bpswap2', 'swap', 'krefine', 'bp-swap'):
        with pytest.raises(RuntimeError, match='graph-matching-toolkit'):
            distance.ged(None, None, algo)
    doc = distance.ged.__doc__
    assert "algo='bpswap'" in doc and 'no toolkit value is claimed' in doc
