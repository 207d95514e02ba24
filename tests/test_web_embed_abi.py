"""Host side of embed-once retrieval for graph-store (Web) models
(include/siamese_web_embed.h): the library exports exactly the header's symbols next to the
unchanged other headers, sg_web_embed_dim / sg_web_embed_ld read the Padding / NTN width off
the path-3 plan, and sg_web_embed / sg_web_score_grid check their arguments before any HIP
call (so all of this runs without a GPU)."""
import ctypes
import os
import re

import pytest

from _embed_fixtures import lib_model, ntn_stack, problem
from graphembedding_amd import _lib
from graphembedding_amd.build import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM_RE = r'^\s*(?:int32_t|int64_t)\s+(sg_\w+)\s*\('   # test_lib_abi.header_symbols
OTHER_HEADERS = {'siamese_hip.h': 'EXPORTED_SYMBOLS', 'siamese_embed.h': 'EMBED_SYMBOLS',
                 'siamese_embed_train.h': 'EMBED_TRAIN_SYMBOLS',
                 'siamese_embed_drop.h': 'EMBED_DROP_SYMBOLS',
                 'siamese_search.h': 'SEARCH_SYMBOLS'}


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def _web(D, K=10, n_max=None, **kw):
    """A path-3 model of Padding / NTN width D."""
    prob = problem(ntn_stack(D, K, **kw), n_max=D, n_lo=5, n_hi=min(D, 40))
    m = lib_model(prob, n_max=n_max or D)
    return m


def test_web_embed_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_web_embed.h')
    assert set(syms) == set(_lib.WEB_EMBED_SYMBOLS), syms
    assert len(_lib.WEB_EMBED_SYMBOLS) == len(set(_lib.WEB_EMBED_SYMBOLS)) == 6
    for s in syms:
        assert hasattr(L, s), s
    assert L.sg_version() == 11000
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.WEB_EMBED_SYMBOLS) & set(other), name
        assert not set(_lib.WEB_EMBED_SYMBOLS) & set(_header_symbols(header)), header
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged


def test_web_embed_dim_and_ld(L):
    for D, ld in ((64, 128), (50, 128), (512, 512)):
        m = _web(D, 16 if D == 512 else 10)
        assert _lib.validate(m)[1] == _lib.PATH_WEB
        assert L.sg_web_embed_dim(m) == D and L.sg_web_embed_ld(m) == ld
        assert _lib.web_embed_dim(m) == D and _lib.web_embed_ld(m) == ld
        assert L.sg_embed_dim(m) == -1                                 # siamese_embed.h: as before
    default = lib_model(problem())                                     # path 1
    c4 = lib_model(problem(n_max=30, n_lo=5, n_hi=30), n_max=32)       # path 2
    assert _lib.validate(default)[1] == 1 and _lib.validate(c4)[1] == 2
    for m in (default, c4, None):
        assert L.sg_web_embed_dim(m) == -1 and L.sg_web_embed_ld(m) == -1
    bad = _web(64)
    bad.num_layers = 1
    assert L.sg_web_embed_dim(bad) == -1 and L.sg_web_embed_ld(bad) == -1
    with pytest.raises(_lib.SiameseHipError):
        _lib.web_embed_dim(default)
    with pytest.raises(_lib.SiameseHipError):
        _lib.web_embed_ld(default)


def _dummy():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def _store(p, n_graphs=4, n_max=40, **null):
    s = _lib.SgCsrStore()
    s.n_graphs, s.n_max, s.max_nnz = n_graphs, n_max, 8
    for f in ('node_off', 'types', 'row_ptr', 'col', 'val'):
        setattr(s, f, None if null.get(f) == 0 else p)
    return s


def test_web_embed_host_validation(L):
    buf, p = _dummy()
    m = _web(64)
    st = _store(p)
    run = lambda model, store, count=2, prm=p, out=p, ws=p: L.sg_web_embed(  # noqa: E731
        model, store, None, count, prm, out, None, ws, None)
    assert run(m, st, count=0, out=None, ws=None) == _lib.SG_OK          # no graphs: no work
    assert run(None, st) == _lib.SG_ERR_ARG
    assert run(m, None) == _lib.SG_ERR_ARG
    assert run(m, st, count=-1) == _lib.SG_ERR_ARG
    for null in ('prm', 'out', 'ws'):
        assert run(m, st, **{null: None}) == _lib.SG_ERR_ARG, null
    for f in ('node_off', 'types', 'row_ptr', 'col', 'val'):
        assert run(m, _store(p, **{f: 0})) == _lib.SG_ERR_ARG, f
    assert run(m, _store(p, n_max=65)) == _lib.SG_ERR_ARG               # store n_max > D
    assert run(_web(64, n_max=48), _store(p, n_max=50)) == _lib.SG_ERR_ARG   # > model n_max
    for other in (lib_model(problem()), lib_model(problem(n_max=30, n_lo=5, n_hi=30), n_max=32)):
        assert run(other, st) == _lib.SG_ERR_UNSUPPORTED
        assert L.sg_web_embed_workspace_bytes(other, 4) == -1
        with pytest.raises(_lib.SiameseHipError):
            _lib.web_embed_workspace_bytes(other, 4)
    assert L.sg_web_embed_workspace_bytes(m, -1) == -1
    assert L.sg_web_embed_workspace_bytes(None, 4) == -1


def _grid_rc(L, m, D=64, q=1, db=1, mm=1, nn=1, prm=1, out=1, ld_q=None, ld_db=None, ld=None,
             ws=1):
    """sg_web_score_grid with dummy non-null pointers: only paths that return before the
    first launch are exercised."""
    buf, p = _dummy()
    return L.sg_web_score_grid(m, p if q else None, D if ld_q is None else ld_q,
                               p if db else None, D if ld_db is None else ld_db, mm, nn,
                               p if prm else None, 0, p if out else None,
                               nn if ld is None else ld, p if ws else None, None)


def test_web_score_grid_host_validation(L):
    ok = _web(64, 16)
    for null in ('q', 'db', 'prm', 'out', 'ws'):
        assert _grid_rc(L, ok, mm=2, nn=3, **{null: 0}) == _lib.SG_ERR_ARG, null
    assert _grid_rc(L, ok, mm=2, nn=3, ld_q=63) == _lib.SG_ERR_ARG       # ld_q < D
    assert _grid_rc(L, ok, mm=2, nn=3, ld_db=63) == _lib.SG_ERR_ARG      # ld_db < D
    assert _grid_rc(L, ok, mm=2, nn=3, ld=2) == _lib.SG_ERR_ARG          # ld_out < n
    assert _grid_rc(L, ok, mm=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, nn=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, None) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, mm=0, q=0, out=0) == _lib.SG_OK               # empty grid: no work
    assert _grid_rc(L, ok, nn=0, db=0, out=0) == _lib.SG_OK
    for other in (lib_model(problem()), lib_model(problem(n_max=30, n_lo=5, n_hi=30), n_max=32),
                  lib_model(problem(dict(num_layers=5, layer_4='Dot')))):
        assert _grid_rc(L, other, D=10) == _lib.SG_ERR_UNSUPPORTED
        assert L.sg_web_score_grid_workspace_bytes(other, 4) == -1
        with pytest.raises(_lib.SiameseHipError):
            _lib.web_score_grid_workspace_bytes(other, 4)
    assert L.sg_web_score_grid_workspace_bytes(ok, -1) == -1
    assert L.sg_web_score_grid_workspace_bytes(None, 4) == -1


def test_web_workspace_queries_are_positive_and_monotone(L):
    for D, K in ((64, 10), (50, 1), (512, 16)):
        m = _web(D, K)
        dq = (D + 1 + 3) // 4 * 4
        prev_e = prev_g = 0
        for size in (0, 1, 7, 64, 300, 4097, 100000):
            e = L.sg_web_embed_workspace_bytes(m, size)
            g = L.sg_web_score_grid_workspace_bytes(m, size)
            assert e > 0 and g > 0
            assert e >= prev_e and g >= prev_g
            assert g >= size * dq * 16 * 4                               # the tables Q [m][Dq][16]
            prev_e, prev_g = e, g
        assert L.sg_web_embed_workspace_bytes(m, 100000) > L.sg_web_embed_workspace_bytes(m, 1)
        assert L.sg_web_score_grid_workspace_bytes(m, 2) > L.sg_web_score_grid_workspace_bytes(m, 1)
