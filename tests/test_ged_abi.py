"""Host side of the device GED bounds (include/siamese_ged.h): the library exports exactly the
header's symbols next to the unchanged other headers' sets, the workspace query, and every
refusal of sg_ged_grid in the header's order before any HIP call (dummy pointers, so all of
this runs without a GPU).  The Python layer's opt-ins default to the synthetic labels."""
import ctypes
import os
import re

import numpy as np
import pytest

from graphembedding_amd import _lib
from graphembedding_amd.build import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM_RE = r'^\s*(?:int32_t|int64_t)\s+(sg_\w+)\s*\('   # test_lib_abi.header_symbols
OTHER_HEADERS = {'siamese_hip.h': 'EXPORTED_SYMBOLS', 'siamese_embed.h': 'EMBED_SYMBOLS',
                 'siamese_embed_train.h': 'EMBED_TRAIN_SYMBOLS',
                 'siamese_embed_drop.h': 'EMBED_DROP_SYMBOLS',
                 'siamese_search.h': 'SEARCH_SYMBOLS',
                 'siamese_web_embed.h': 'WEB_EMBED_SYMBOLS',
                 'siamese_web_search.h': 'WEB_SEARCH_SYMBOLS',
                 'siamese_web_embed_train.h': 'WEB_EMBED_TRAIN_SYMBOLS',
                 'siamese_web_embed_drop.h': 'WEB_EMBED_DROP_SYMBOLS',
                 'siamese_eval.h': 'EVAL_SYMBOLS', 'siamese_dot_embed.h': 'DOT_EMBED_SYMBOLS'}
A, U, OK = _lib.SG_ERR_ARG, _lib.SG_ERR_UNSUPPORTED, _lib.SG_OK


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def test_ged_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_ged.h')
    assert set(syms) == set(_lib.GED_SYMBOLS), syms
    assert len(_lib.GED_SYMBOLS) == len(set(_lib.GED_SYMBOLS)) == 2
    for s in syms:
        assert hasattr(L, s), s
    for fn in ('ged_grid_workspace_bytes', 'ged_grid'):
        assert callable(getattr(_lib, fn)), fn
    assert L.sg_version() == 11000
    assert "symbols' presence" in open(os.path.join(ROOT, 'include', 'siamese_ged.h')).read()


def test_ged_symbols_are_disjoint_from_the_other_headers():
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.GED_SYMBOLS) & set(other), name
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged


def test_ged_unit_is_a_source_of_the_library():
    from graphembedding_amd import build
    assert 'sg_ged.hip' in build.SOURCES
    assert os.path.isfile(os.path.join(build.CSRC, 'sg_ged.hip'))


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _rc(L, m=3, n=5, ld=None, n_graphs=8, n_max=10, both=1, **null):
    """sg_ged_grid with dummy non-null pointers (name=0 passes NULL): only paths that return
    before the first launch are exercised."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_ged_grid(p('adj'), p('types'), p('sn'), n_graphs, n_max, p('q'), m, p('db'), n,
                         both, p('ub'), n if ld is None else ld, p('lb'), p('map'), p('status'),
                         p('ws'), None)


def test_ged_argument_rules(L):
    """The header's table, rule by rule and in its order: a later rule's violation never hides
    an earlier one's.  `adj=0` (the last rule) marks calls that pass every other rule."""
    ws = L.sg_ged_grid_workspace_bytes
    # 1. negative sizes, before anything else
    assert _rc(L, m=-1) == A and ws(-1, 5, 10) == -1
    assert _rc(L, n=-1) == A and ws(3, -1, 10) == -1
    assert _rc(L, ld=-1) == A
    assert _rc(L, m=-1, n_max=33) == A
    assert _rc(L, ld=-1, n_max=33) == A
    # 2. n_graphs < 0, n_max < 1
    assert _rc(L, n_graphs=-1) == A
    assert _rc(L, n_graphs=-1, n_max=33) == A
    assert _rc(L, n_max=0) == A and ws(3, 5, 0) == -1
    assert _rc(L, n_max=-4) == A and ws(3, 5, -4) == -1
    assert _rc(L, n_graphs=0, adj=0) == A                # an empty store passes on (all ids bad)
    # 3. n_max > 32
    assert _rc(L, n_max=33) == U and ws(3, 5, 33) == -1
    assert _rc(L, n_max=33, ld=2) == U                   # before ld < n
    assert _rc(L, n_max=33, m=0) == U                    # before the empty call
    assert _rc(L, n_max=32, adj=0) == A and ws(3, 5, 32) == 4 * 8 * 68
    assert _rc(L, n_max=1, adj=0) == A and ws(3, 5, 1) == 4 * 8 * 4
    # 4. grid sizes
    big = (1 << 24) + 1
    assert _rc(L, m=big) == U and ws(big, 5, 10) == -1
    assert _rc(L, n=big, ld=big) == U and ws(3, big, 10) == -1
    assert _rc(L, m=1 << 24, n=257, ld=257) == U and ws(1 << 24, 257, 10) == -1
    assert _rc(L, m=1 << 24, n=256, ld=256, adj=0) == A
    assert ws(1 << 24, 256, 10) == 4 * ((1 << 24) + 256) * 24
    assert _rc(L, m=big, ld=2) == U                      # before ld < n
    # 5. ld < n
    assert _rc(L, ld=4) == A
    assert _rc(L, ld=4, both=2) == A
    assert _rc(L, m=0, ld=4) == A                        # before the empty call
    assert _rc(L, ld=9, adj=0) == A                      # ld > n is fine: on to the pointers
    # 6. both_orders
    assert _rc(L, both=2) == A
    assert _rc(L, both=-1) == A
    assert _rc(L, m=0, both=2) == A
    # 7. empty grids: no work, whatever the pointers
    assert _rc(L, m=0, adj=0, types=0, sn=0, ub=0, ws=0) == OK
    assert _rc(L, n=0, ld=0, adj=0, types=0, sn=0, ub=0, ws=0) == OK
    assert ws(0, 5, 10) == 0 and ws(3, 0, 10) == 0
    # 8. the required pointers; q_idx, db_idx, lb_out, map_out and status_out may be NULL
    for null in ('adj', 'types', 'sn', 'ub', 'ws'):
        assert _rc(L, **{null: 0}) == A, null
    assert _rc(L, both=0, q=0, db=0, lb=0, map=0, status=0, adj=0) == A
    # the workspace of the default shapes: (m + n) entries of 2 n_max + 1 words, padded to 16 B
    assert ws(3, 5, 10) == 4 * 8 * 24
    assert ws(700, 700, 10) == 4 * 1400 * 24
    with pytest.raises(_lib.SiameseHipError, match='sg_ged_grid_workspace_bytes'):
        _lib.ged_grid_workspace_bytes(3, 5, 33)
    assert _lib.ged_grid_workspace_bytes(3, 5, 10) == 768


def test_label_opt_ins_default_to_synthetic():
    import inspect

    from graphembedding_amd import allpairs, data
    from graphembedding_amd.config import DEFAULTS, Flags
    assert Flags().ged_labels == 'synthetic' == DEFAULTS['ged_labels']
    assert inspect.signature(allpairs.load_graph_set).parameters['ged'].default == 'synthetic'
    gs = allpairs.load_graph_set('syn_aids80nef')
    assert np.array_equal(gs.ged, data.synthetic_ged_matrix(gs.graphs))
    with pytest.raises(RuntimeError, match='Unknown ged labels'):
        allpairs.load_graph_set('syn_aids80nef', ged='hungarian')


def test_distance_ged_computes_only_bp():
    from graphembedding_amd import distance
    for algo in ('astar', 'beam80', 'hungarian', 'vj'):
        with pytest.raises(RuntimeError, match='graph-matching-toolkit'):
            distance.ged(None, None, algo)
    doc = distance.ged.__doc__
    assert "'bp'" in doc and "not 'hungarian'" in doc and 'not been checked' in doc


def test_store_of_graphs_limits_and_types():
    import networkx as nx

    from graphembedding_amd.ged import store_of_graphs
    a = nx.path_graph(3)
    nx.set_node_attributes(a, {0: 'C', 1: 'N', 2: 'C'}, 'type')
    b = nx.cycle_graph(4)
    nx.set_node_attributes(b, 'N', 'type')
    s = store_of_graphs([a, b])
    assert s.n_max == 4 and s.n.tolist() == [3, 4]
    assert s.types[0, :3].tolist() == [0, 1, 0] and s.types[1].tolist() == [1, 1, 1, 1]
    plain = store_of_graphs([nx.path_graph(2), nx.path_graph(5)])      # no 'type': one type
    assert plain.n_max == 5 and not plain.types.any()
    with pytest.raises(_lib.SiameseHipError, match='at most 32 nodes'):
        store_of_graphs([nx.path_graph(33)])
