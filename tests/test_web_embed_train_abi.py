"""Host side of embed-once training for graph-store (Web) models
(include/siamese_web_embed_train.h): the library exports exactly the header's symbols next to
the unchanged other headers, both calls refuse what they do not serve with the documented
codes in the documented order before any HIP call (so all of this runs without a GPU), and
the grid's workspace query follows the formula of the header."""
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
                 'siamese_search.h': 'SEARCH_SYMBOLS',
                 'siamese_web_embed.h': 'WEB_EMBED_SYMBOLS',
                 'siamese_web_search.h': 'WEB_SEARCH_SYMBOLS'}
MAX_ROWS = 1 << 29


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def _web(D, K=10, keep_prob=1.0, **kw):
    """A path-3 model of Padding / NTN width D, by default without dropout (keep_prob 1)."""
    prob = problem(ntn_stack(D, K, **kw), n_max=D, n_lo=5, n_hi=min(D, 40))
    return lib_model(prob, n_max=D, keep_prob=keep_prob)


def _others():
    """Models sg_web_score_grid refuses: path 1, path 2, the Dot head, K = 17."""
    return (lib_model(problem()), lib_model(problem(n_max=30, n_lo=5, n_hi=30), n_max=32),
            lib_model(problem(dict(num_layers=5, layer_4='Dot'))), _web(64, 17))


def _dummy():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


_BUF, _P = _dummy()


def _grid_rc(L, m, D=64, mm=2, nn=3, ld_q=None, ld_db=None, ld_lab=None, ld_s=None, ld_gq=None,
             ld_gdb=None, bt=None, **null):
    """sg_web_score_grid_fwd_bwd with dummy non-null pointers (name=0 passes NULL): only
    paths that return before the first launch are exercised."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    d = lambda v: D if v is None else v                    # noqa: E731
    return L.sg_web_score_grid_fwd_bwd(
        m, p('q'), d(ld_q), p('db'), d(ld_db), mm, nn, p('prm'), p('lab'),
        nn if ld_lab is None else ld_lab, mm * nn if bt is None else bt, p('ys'), 1, p('s'),
        nn if ld_s is None else ld_s, p('gq'), d(ld_gq), p('gdb'), d(ld_gdb), p('grad'),
        p('loss'), p('ws'), None)


def _fwd_grid_rc(L, m, D=64):
    return L.sg_web_score_grid(m, _P, D, _P, D, 1, 1, _P, 0, _P, 1, _P, None)


def _store(n_graphs=4, n_max=40, **null):
    s = _lib.SgCsrStore()
    s.n_graphs, s.n_max, s.max_nnz = n_graphs, n_max, 8
    for f in ('node_off', 'types', 'row_ptr', 'col', 'val'):
        setattr(s, f, None if null.get(f) == 0 else _P)
    return s


def _bwd_rc(L, m, store, count=2, ld_g=64, **null):
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_web_embed_bwd(m, store, None, count, p('prm'), p('g'), ld_g, p('grad'), None,
                              p('ws'), None)


def test_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_web_embed_train.h')
    assert set(syms) == set(_lib.WEB_EMBED_TRAIN_SYMBOLS), syms
    assert len(_lib.WEB_EMBED_TRAIN_SYMBOLS) == len(set(_lib.WEB_EMBED_TRAIN_SYMBOLS)) == 4
    for s in syms:
        assert hasattr(L, s), s
    assert L.sg_version() == 11000
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.WEB_EMBED_TRAIN_SYMBOLS) & set(other), name
        assert not set(_lib.WEB_EMBED_TRAIN_SYMBOLS) & set(_header_symbols(header)), header
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged


def test_grid_refusal_order_and_codes(L):
    ok = _web(64, 16)
    # every model the forward grid refuses: the same code, before anything else is looked at
    for other in _others():
        want = _fwd_grid_rc(L, other, D=10)
        assert want == _lib.SG_ERR_UNSUPPORTED
        assert _grid_rc(L, other, D=10) == want
        assert _grid_rc(L, other, D=10, mm=MAX_ROWS + 1, q=0) == want    # model first
        assert L.sg_web_score_grid_bwd_workspace_bytes(other, 4, 4) == -1
        with pytest.raises(_lib.SiameseHipError):
            _lib.web_score_grid_bwd_workspace_bytes(other, 4, 4)
    assert _grid_rc(L, None) == _lib.SG_ERR_ARG
    # a Web model with dropout: refused by both calls and both queries
    dropped = _web(64, 16, keep_prob=0.9)
    assert _fwd_grid_rc(L, dropped) != _lib.SG_ERR_UNSUPPORTED           # retrieval serves it
    assert _grid_rc(L, dropped) == _lib.SG_ERR_UNSUPPORTED
    assert _grid_rc(L, dropped, mm=0) == _lib.SG_ERR_UNSUPPORTED         # before the empty grid
    assert _bwd_rc(L, dropped, _store()) == _lib.SG_ERR_UNSUPPORTED
    assert _bwd_rc(L, dropped, _store(), count=0) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_web_score_grid_bwd_workspace_bytes(dropped, 4, 4) == -1
    assert L.sg_web_embed_bwd_workspace_bytes(dropped, 4) == -1
    # sizes
    assert _grid_rc(L, ok, mm=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, nn=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, mm=MAX_ROWS + 1) == _lib.SG_ERR_UNSUPPORTED
    assert _grid_rc(L, ok, nn=MAX_ROWS + 1) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_web_score_grid_bwd_workspace_bytes(ok, MAX_ROWS + 1, 4) == -1
    assert L.sg_web_score_grid_bwd_workspace_bytes(ok, 4, MAX_ROWS + 1) == -1
    assert L.sg_web_score_grid_bwd_workspace_bytes(ok, -1, 4) == -1
    assert L.sg_web_score_grid_bwd_workspace_bytes(None, 4, 4) == -1
    # the empty grid: no work, nothing is looked at
    assert _grid_rc(L, ok, mm=0, q=0, gq=0, ws=0) == _lib.SG_OK
    assert _grid_rc(L, ok, nn=0, db=0, gdb=0, ws=0) == _lib.SG_OK
    # pointers and strides
    for null in ('q', 'db', 'prm', 'gq', 'gdb', 'grad', 'ws', 'ys'):
        assert _grid_rc(L, ok, **{null: 0}) == _lib.SG_ERR_ARG, null
    for ld in ('ld_q', 'ld_db', 'ld_gq', 'ld_gdb'):
        assert _grid_rc(L, ok, **{ld: 63}) == _lib.SG_ERR_ARG, ld
    assert _grid_rc(L, ok, ld_s=2) == _lib.SG_ERR_ARG                    # ld_s < n
    aligned = _web(64, 16, loss_mode='aligned')
    assert _grid_rc(L, aligned, lab=0) == _lib.SG_ERR_ARG
    assert _grid_rc(L, aligned, ld_lab=2) == _lib.SG_ERR_ARG
    assert _grid_rc(L, aligned, bt=0) == _lib.SG_ERR_ARG


def test_embed_bwd_host_validation(L):
    m = _web(64)
    st = _store()
    assert _bwd_rc(L, None, st) == _lib.SG_ERR_ARG
    assert _bwd_rc(L, m, None) == _lib.SG_ERR_ARG
    assert _bwd_rc(L, m, st, count=-1) == _lib.SG_ERR_ARG
    for null in ('prm', 'g', 'grad', 'ws'):
        assert _bwd_rc(L, m, st, **{null: 0}) == _lib.SG_ERR_ARG, null
    assert _bwd_rc(L, m, st, ld_g=63) == _lib.SG_ERR_ARG                 # ld_g < D
    for f in ('node_off', 'types', 'row_ptr', 'col', 'val'):
        assert _bwd_rc(L, m, _store(**{f: 0})) == _lib.SG_ERR_ARG, f
    assert _bwd_rc(L, m, _store(n_max=65)) == _lib.SG_ERR_ARG            # store n_max > D
    assert _bwd_rc(L, m, st, count=MAX_ROWS + 1) == _lib.SG_ERR_UNSUPPORTED
    for other in _others()[:3]:
        assert _bwd_rc(L, other, st) == _lib.SG_ERR_UNSUPPORTED
        assert L.sg_web_embed_bwd_workspace_bytes(other, 4) == -1
        with pytest.raises(_lib.SiameseHipError):
            _lib.web_embed_bwd_workspace_bytes(other, 4)
    assert L.sg_web_embed_bwd_workspace_bytes(m, -1) == -1
    assert L.sg_web_embed_bwd_workspace_bytes(None, 4) == -1
    prev = 0
    for count in (0, 1, 7, 300, 1024, 1025, 100000):
        b = L.sg_web_embed_bwd_workspace_bytes(m, count)
        assert b > 0 and b >= prev
        prev = b
    # chunks of 1024 entries: the workspace stops growing
    assert L.sg_web_embed_bwd_workspace_bytes(m, 1024) == L.sg_web_embed_bwd_workspace_bytes(m, 10 ** 6)


def _up64(x):
    return (x + 63) & ~63


def _grid_ws_formula(D, m, n):
    """The formula of include/siamese_web_embed_train.h."""
    dq = (D + 1 + 3) // 4 * 4
    n64 = _up64(n)
    gm = min(min(m, 256) * n64 * 16, max(1 << 23, n64 * 16))
    return 4 * (2 * _up64(m * dq * 16) + _up64(gm) + _up64((n64 // 64 + 512) * 32)) + 256


def test_grid_workspace_formula(L):
    sizes = (0, 1, 5, 63, 64, 65, 300, 4096, 4097, 100000)
    for D, K in ((33, 10), (50, 1), (64, 10), (512, 16)):
        model = _web(D, K)
        for m in sizes:
            prev = 0
            for n in sizes:
                b = L.sg_web_score_grid_bwd_workspace_bytes(model, m, n)
                assert b == _grid_ws_formula(D, m, n), (D, m, n)
                assert b >= prev                                         # monotone in n
                prev = b
        for n in sizes:
            col = [L.sg_web_score_grid_bwd_workspace_bytes(model, m, n) for m in sizes]
            assert col == sorted(col), (D, n)                            # monotone in m
    big = L.sg_web_score_grid_bwd_workspace_bytes(_web(512, 16), 4096, 4096)
    assert 0 < big < 512 << 20, big
    # no term in m·n·D, and the m·n term is capped: doubling m adds the tables only
    m512 = _web(512, 16)
    d = L.sg_web_score_grid_bwd_workspace_bytes(m512, 8192, 4096) - big
    assert d == 4 * 2 * 4096 * 516 * 16


def test_other_training_calls_still_refuse_web_models(L):
    m = _web(64)
    assert _lib.validate(m)[1] == _lib.PATH_WEB
    assert L.sg_score_grid_fwd_bwd(m, _P, _P, 2, 3, _P, _P, 3, 6, _P, 1, _P, 3, _P, _P, _P, _P, _P,
                                   None) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_score_grid_bwd_workspace_bytes(m, 2, 3) == -1
    assert L.sg_embed_bwd(m, _P, _P, _P, 4, 64, None, 2, _P, _P, _P, None, _P,
                          None) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_embed_bwd_workspace_bytes(m, 2) == -1
