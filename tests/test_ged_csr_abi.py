"""Host side of the graph-store GED bounds (include/siamese_ged_csr.h): the library exports the
header's two symbols next to every other header's unchanged set, the workspace query, and every
refusal of sg_csr_ged_grid in the header's order before any HIP call (dummy pointers, so all of
this runs without a GPU); csr_store_of_graphs' limits."""
import ctypes
import os
import re

import networkx as nx
import pytest

from graphembedding_amd import _lib
from graphembedding_amd.build import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM_RE = r'^\s*(?:int32_t|int64_t)\s+(sg_\w+)\s*\('
OTHER_HEADERS = {'siamese_hip.h': 'EXPORTED_SYMBOLS', 'siamese_embed.h': 'EMBED_SYMBOLS',
                 'siamese_embed_train.h': 'EMBED_TRAIN_SYMBOLS',
                 'siamese_embed_drop.h': 'EMBED_DROP_SYMBOLS',
                 'siamese_search.h': 'SEARCH_SYMBOLS',
                 'siamese_web_embed.h': 'WEB_EMBED_SYMBOLS',
                 'siamese_web_search.h': 'WEB_SEARCH_SYMBOLS',
                 'siamese_web_embed_train.h': 'WEB_EMBED_TRAIN_SYMBOLS',
                 'siamese_web_embed_drop.h': 'WEB_EMBED_DROP_SYMBOLS',
                 'siamese_eval.h': 'EVAL_SYMBOLS', 'siamese_dot_embed.h': 'DOT_EMBED_SYMBOLS',
                 'siamese_ged.h': 'GED_SYMBOLS', 'siamese_ged_exact.h': 'GED_EXACT_SYMBOLS',
                 'siamese_ged_beam.h': 'GED_BEAM_SYMBOLS'}
A, U, OK = _lib.SG_ERR_ARG, _lib.SG_ERR_UNSUPPORTED, _lib.SG_OK


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def test_csr_ged_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_ged_csr.h')
    assert set(syms) == set(_lib.GED_CSR_SYMBOLS), syms
    assert len(_lib.GED_CSR_SYMBOLS) == len(set(_lib.GED_CSR_SYMBOLS)) == 2
    for s in syms:
        assert hasattr(L, s), s
    for fn in ('csr_ged_grid_workspace_bytes', 'csr_ged_grid'):
        assert callable(getattr(_lib, fn)), fn
    src = open(os.path.join(ROOT, 'include', 'siamese_ged_csr.h')).read()
    assert "symbols' presence" in src and 'sg_ged_grid' not in src and 'ascending' in src
    from graphembedding_amd import build
    assert 'sg_ged_csr.hip' in build.SOURCES


def test_csr_ged_symbols_are_disjoint_from_the_other_headers():
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.GED_CSR_SYMBOLS) & set(other), name
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _rc(L, m=3, n=5, ld=None, n_graphs=8, n_max=100, both=1, store=True, **null):
    """sg_csr_ged_grid with dummy non-null pointers (name=0 passes NULL): only paths that return
    before the first launch are exercised."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    st = _lib.SgCsrStore()
    st.n_graphs, st.n_max, st.max_nnz = n_graphs, n_max, 0
    st.node_off, st.types, st.row_ptr = p('node_off'), p('types'), p('row_ptr')
    st.col, st.val = p('col'), p('val')
    return L.sg_csr_ged_grid(ctypes.byref(st) if store else None, p('q'), m, p('db'), n, both,
                             p('ub'), n if ld is None else ld, p('lb'), p('map'), p('status'),
                             p('ws'), None)


def test_csr_ged_argument_rules(L):
    """The header's table, rule by rule and in its order.  `val=0` (the last rule) marks calls
    that pass every other rule."""
    ws = L.sg_csr_ged_grid_workspace_bytes
    # 1. negative sizes, before anything else
    assert _rc(L, m=-1) == A and ws(-1, 5, 100) == -1
    assert _rc(L, n=-1) == A and ws(3, -1, 100) == -1
    assert _rc(L, ld=-1) == A
    assert _rc(L, m=-1, n_max=513) == A and _rc(L, ld=-1, n_max=513) == A
    # 2. n_graphs < 0, n_max < 1
    assert _rc(L, n_graphs=-1) == A and _rc(L, n_graphs=-1, n_max=513) == A
    assert _rc(L, n_max=0) == A and ws(3, 5, 0) == -1
    assert _rc(L, n_max=-4) == A and ws(3, 5, -4) == -1
    assert _rc(L, n_graphs=0, val=0) == A                 # an empty store passes on (all ids bad)
    # 3. n_max > 512
    assert _rc(L, n_max=513) == U and ws(3, 5, 513) == -1
    assert _rc(L, n_max=513, ld=2) == U                   # before ld < n
    assert _rc(L, n_max=513, m=0) == U                    # before the empty call
    assert _rc(L, n_max=512, val=0) == A and ws(3, 5, 512) == 4 * 8 * 516
    assert _rc(L, n_max=33, val=0) == A and ws(3, 5, 33) == 4 * 8 * 36
    assert _rc(L, n_max=1, val=0) == A and ws(3, 5, 1) == 4 * 8 * 4
    # 4. grid sizes
    big = (1 << 24) + 1
    assert _rc(L, m=big) == U and ws(big, 5, 100) == -1
    assert _rc(L, n=big, ld=big) == U and ws(3, big, 100) == -1
    assert _rc(L, m=1 << 24, n=257, ld=257) == U and ws(1 << 24, 257, 100) == -1
    assert _rc(L, m=1 << 24, n=256, ld=256, val=0) == A
    assert _rc(L, m=big, ld=2) == U                       # before ld < n
    # 5. ld < n
    assert _rc(L, ld=4) == A and _rc(L, ld=4, both=2) == A
    assert _rc(L, m=0, ld=4) == A                         # before the empty call
    assert _rc(L, ld=9, val=0) == A                       # ld > n is fine: on to the pointers
    # 6. both_orders
    assert _rc(L, both=2) == A and _rc(L, both=-1) == A and _rc(L, m=0, both=2) == A
    # 7. empty grids: no work, whatever the pointers
    assert _rc(L, m=0, node_off=0, types=0, row_ptr=0, col=0, val=0, ub=0, ws=0) == OK
    assert _rc(L, n=0, ld=0, store=False, ub=0, ws=0) == OK
    assert ws(0, 5, 100) == 0 and ws(3, 0, 100) == 0
    # 8. the store and the required pointers; q_idx, db_idx, lb_out, map_out, status_out may be NULL
    assert _rc(L, store=False) == A
    assert _rc(L, store=False, m=big) == U and _rc(L, store=False, ld=2) == A
    for null in ('node_off', 'types', 'row_ptr', 'col', 'val', 'ub', 'ws'):
        assert _rc(L, **{null: 0}) == A, null
    assert _rc(L, both=0, q=0, db=0, lb=0, map=0, status=0, val=0) == A
    # the workspace: (m + n) entries of n_max + 2 words, padded to 16 B
    assert ws(3, 5, 100) == 4 * 8 * 104 and ws(700, 700, 288) == 4 * 1400 * 292
    with pytest.raises(_lib.SiameseHipError, match='sg_csr_ged_grid_workspace_bytes'):
        _lib.csr_ged_grid_workspace_bytes(3, 5, 513)
    assert _lib.csr_ged_grid_workspace_bytes(3, 5, 100) == 3328


def test_store_builders_limits():
    from graphembedding_amd.ged import csr_store_of_graphs, store_of_graphs
    a = nx.path_graph(33)
    nx.set_node_attributes(a, {v: 'CN'[v % 2] for v in a}, 'type')
    s = csr_store_of_graphs([a, nx.Graph(a.subgraph(range(3)))])
    assert s.n_max == 33 and s.n.tolist() == [33, 3] and s.types[:4].tolist() == [0, 1, 0, 1]
    assert s.types[33:].tolist() == [0, 1, 0]
    for r in range(36):                                   # columns strictly ascending per row
        c = s.col[s.row_ptr[r]:s.row_ptr[r + 1]]
        assert (c[1:] > c[:-1]).all()
    plain = csr_store_of_graphs([nx.path_graph(40)])      # no 'type': one type
    assert plain.n_max == 40 and not plain.types.any()
    assert csr_store_of_graphs([nx.path_graph(512)]).n_max == 512
    with pytest.raises(_lib.SiameseHipError, match='at most 512 nodes'):
        csr_store_of_graphs([nx.path_graph(513)])
    with pytest.raises(_lib.SiameseHipError, match='at most 32 nodes'):
        store_of_graphs([nx.path_graph(33)])


def test_search_options_keep_refusing_above_32_nodes():
    """The graph-store route has the bounds only: with exact_budget or beam_width a 33-node graph
    is refused where it was, by store_of_graphs, before any device call."""
    from graphembedding_amd import distance
    from graphembedding_amd.ged import ged_matrix, ged_pair
    g = nx.path_graph(33)
    for kw in (dict(exact_budget=1), dict(beam_width=1)):
        with pytest.raises(_lib.SiameseHipError, match='at most 32 nodes'):
            ged_pair(g, g, **kw)
        with pytest.raises(_lib.SiameseHipError, match='at most 32 nodes'):
            ged_matrix([g, g], **kw)
    for algo in ('exact', 'lbeam80'):
        with pytest.raises(_lib.SiameseHipError, match='at most 32 nodes'):
            distance.ged(g, g, algo)
