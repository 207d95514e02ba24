"""Host side of embed-once search for graph-store (Web) models
(include/siamese_web_search.h): the library exports exactly the header's symbols next to the
unchanged other headers' sets, sg_web_search_topk refuses what sg_web_score_grid and
sg_search_topk refuse, in that order and before any HIP call, and its workspace holds nothing
proportional to m·n (so all of this runs without a GPU)."""
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
                 'siamese_web_embed.h': 'WEB_EMBED_SYMBOLS'}


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def _web(D, K=10, **kw):
    """A path-3 model of Padding / NTN width D."""
    prob = problem(ntn_stack(D, K, **kw), n_max=D, n_lo=5, n_hi=min(D, 40))
    return lib_model(prob, n_max=D)


def test_web_search_header_symbols_are_exported(L):
    assert hasattr(_lib, 'WEB_SEARCH_SYMBOLS')
    syms = _header_symbols('siamese_web_search.h')
    assert set(syms) == set(_lib.WEB_SEARCH_SYMBOLS), syms
    assert len(_lib.WEB_SEARCH_SYMBOLS) == len(set(_lib.WEB_SEARCH_SYMBOLS)) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert L.sg_version() == 11000
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.WEB_SEARCH_SYMBOLS) & set(other), name
        assert not set(_lib.WEB_SEARCH_SYMBOLS) & set(_header_symbols(header)), header
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged


def _dummy():
    buf = (ctypes.c_float * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p).value


def _rc(L, m, D=64, q=1, db=1, mm=2, nn=100, prm=1, k=5, seg=0, idx=1, val=1, ws=1, ld_q=None,
        ld_db=None):
    """sg_web_search_topk with dummy non-null pointers: only paths that return before the
    first launch are exercised."""
    buf, p = _dummy()
    return L.sg_web_search_topk(m, p if q else None, D if ld_q is None else ld_q,
                                p if db else None, D if ld_db is None else ld_db, mm, nn,
                                p if prm else None, 1, k, 1, seg, p if idx else None,
                                p if val else None, p if ws else None, None)


def _grid_rc(L, m, D=64, mm=2, nn=100):
    """What sg_web_score_grid says of the model, with the same dummy pointers."""
    buf, p = _dummy()
    return L.sg_web_score_grid(m, p, D, p, D, mm, nn, p, 1, p, nn, p, None)


def test_web_search_refuses_the_models_the_grid_refuses(L):
    others = {'path1': lib_model(problem()),
              'path2': lib_model(problem(n_max=30, n_lo=5, n_hi=30), n_max=32),
              'dot': lib_model(problem(dict(num_layers=5, layer_4='Dot')))}
    for name, m in others.items():
        assert _lib.validate(m)[1] != _lib.PATH_WEB, name
        want = _grid_rc(L, m, D=10)
        assert want != _lib.SG_OK, name
        assert _rc(L, m, D=10) == want, name
        assert L.sg_web_search_topk_workspace_bytes(m, 2, 100, 5, 0) == -1, name
        with pytest.raises(_lib.SiameseHipError):
            _lib.web_search_workspace_bytes(m, 2, 100, 5)
    bad = _web(64)
    bad.num_layers = 1                                   # not a valid model at all
    assert _rc(L, bad) == _grid_rc(L, bad) != _lib.SG_OK
    assert L.sg_web_search_topk_workspace_bytes(bad, 2, 100, 5, 0) == -1
    k17 = _web(64, 17)                                   # the graph-store stack, 17 feature maps
    assert _rc(L, k17) == _grid_rc(L, k17) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_web_search_topk_workspace_bytes(k17, 2, 100, 5, 0) == -1
    assert _rc(L, None) == _grid_rc(L, None) == _lib.SG_ERR_ARG
    assert L.sg_web_search_topk_workspace_bytes(None, 2, 100, 5, 0) == -1
    # the model comes first: a refused model with a refused k reports the model
    assert _rc(L, k17, k=0) == _lib.SG_ERR_UNSUPPORTED
    assert _rc(L, others['path1'], D=10, k=0) == _grid_rc(L, others['path1'], D=10)


def test_web_search_host_validation(L):
    for m, D in ((_web(64, 16), 64), (_web(50, 1), 50), (_web(512, 16), 512)):
        assert _lib.validate(m)[1] == _lib.PATH_WEB
        rc = lambda **kw: _rc(L, m, D=D, **kw)           # noqa: E731
        assert rc(k=0) == _lib.SG_ERR_ARG
        assert rc(k=-3) == _lib.SG_ERR_ARG
        assert rc(nn=10, k=11) == _lib.SG_ERR_ARG                  # k > n
        assert rc(nn=0, k=1) == _lib.SG_ERR_ARG                    # k > n = 0
        assert rc(nn=100, k=65) == _lib.SG_ERR_UNSUPPORTED         # k > 64
        assert rc(nn=10, k=65) == _lib.SG_ERR_UNSUPPORTED          # as sg_topk_rows
        for seg in (100, -64, 1, 63, 65):
            assert rc(seg=seg) == _lib.SG_ERR_ARG, seg
            assert L.sg_web_search_topk_workspace_bytes(m, 2, 100, 5, seg) == -1, seg
        assert rc(mm=-1) == _lib.SG_ERR_ARG
        assert rc(nn=-1) == _lib.SG_ERR_ARG
        assert rc(mm=(1 << 29) + 1) == _lib.SG_ERR_UNSUPPORTED
        assert rc(nn=(1 << 29) + 1) == _lib.SG_ERR_UNSUPPORTED
        for null in ('q', 'db', 'prm', 'idx', 'ws'):
            assert rc(**{null: 0}) == _lib.SG_ERR_ARG, null
        assert rc(ld_q=D - 1) == _lib.SG_ERR_ARG                   # ld_q < D
        assert rc(ld_db=D - 1) == _lib.SG_ERR_ARG                  # ld_db < D
        assert rc(ld_q=0) == _lib.SG_ERR_ARG and rc(ld_db=-5) == _lib.SG_ERR_ARG
        # k and seg_cols come before the pointers
        assert rc(k=65, q=0) == _lib.SG_ERR_UNSUPPORTED
        # no rows: no work, whatever the pointers; the argument checks still come first
        assert rc(mm=0, q=0, idx=0, val=0, ws=0) == _lib.SG_OK
        assert rc(mm=0, q=0, ld_q=0) == _lib.SG_OK
        assert rc(mm=0, k=0) == _lib.SG_ERR_ARG
        assert rc(mm=0, k=65) == _lib.SG_ERR_UNSUPPORTED
        assert rc(mm=0, seg=100) == _lib.SG_ERR_ARG
        assert rc(mm=0, nn=(1 << 29) + 1) == _lib.SG_ERR_UNSUPPORTED
        for k, seg in ((0, 0), (65, 0), (101, 0), (5, 100)):
            assert L.sg_web_search_topk_workspace_bytes(m, 2, 100, k, seg) == -1, (k, seg)
        assert L.sg_web_search_topk_workspace_bytes(m, -1, 100, 5, 0) == -1
        assert L.sg_web_search_topk_workspace_bytes(m, (1 << 29) + 1, 100, 5, 0) == -1
        assert L.sg_web_search_topk_workspace_bytes(m, 0, 100, 5, 0) >= 0


def _formula(D, m, n, k, seg):
    """The workspace formula of include/siamese_web_search.h."""
    dq = (D + 4) & ~3
    S = -(-n // seg)
    return ((m * dq * 16 * 4 + 255) & ~255) + S * m * k * 8 + S * m * k * 4 + 256


def test_web_search_workspace_does_not_grow_with_m_times_n(L):
    """256 queries against 2^20 database rows at D = 512, K = 16, k = 10, segments of 4096
    columns: the tables (8.5 MB) plus 256 segments x 256 x 10 candidates of 12 B, where the
    two-call path needs the 1 GiB matrix."""
    D = 512
    model = _web(D, 16)
    m, n, k, seg = 256, 1 << 20, 10, 4096
    b = L.sg_web_search_topk_workspace_bytes(model, m, n, k, seg)
    assert b == _formula(D, m, n, k, seg) == _lib.web_search_workspace_bytes(model, m, n, k, seg)
    tables = m * 516 * 16 * 4
    assert tables <= L.sg_web_score_grid_workspace_bytes(model, m)
    assert b == tables + 256 * m * k * 12 + 256          # m · Dq · 64 is a multiple of 256
    assert 0 < b < 20 << 20 < m * n * 4 == 1 << 30, b
    # the library's own choice: sized for its shortest segments, 1024 columns
    b0 = L.sg_web_search_topk_workspace_bytes(model, m, n, k, 0)
    assert b0 == _formula(D, m, n, k, 1024) < 48 << 20
    # a segment longer than the database is one segment
    one = L.sg_web_search_topk_workspace_bytes(model, 4, 100, 5, 128)
    assert L.sg_web_search_topk_workspace_bytes(model, 4, 100, 5, 1 << 40) == one
    assert one == _formula(D, 4, 100, 5, 128)
    # other widths, D % 4 != 0 among them
    for D2, K2 in ((64, 10), (50, 1), (33, 10)):
        mod = _web(D2, K2)
        for mm, nn, kk, sg in ((1, 1, 1, 64), (7, 1000, 64, 64), (300, 5000, 10, 1024)):
            assert L.sg_web_search_topk_workspace_bytes(mod, mm, nn, kk, sg) == \
                _formula(D2, mm, nn, kk, sg), (D2, mm, nn, kk, sg)


def test_web_search_workspace_is_monotone(L):
    for D, K in ((64, 10), (512, 16)):
        model = _web(D, K)
        for seg in (0, 64, 4096):
            by_m = [L.sg_web_search_topk_workspace_bytes(model, m, 100000, 10, seg)
                    for m in (0, 1, 2, 5, 64, 1000, 100000)]
            by_k = [L.sg_web_search_topk_workspace_bytes(model, 64, 100000, k, seg)
                    for k in (1, 2, 10, 63, 64)]
            assert by_m[0] >= 0 and by_m == sorted(by_m) and len(set(by_m)) == len(by_m), by_m
            assert by_k[0] > 0 and by_k == sorted(by_k) and len(set(by_k)) == len(by_k), by_k


def test_search_still_refuses_web_models(L):
    """siamese_search.h keeps its own domain: the new call does not widen sg_search_topk."""
    web = _web(64)
    buf, p = _dummy()
    assert L.sg_search_topk(web, p, p, 2, 100, p, 1, 5, 1, 0, p, p, p, None) == \
        _lib.SG_ERR_UNSUPPORTED
    assert L.sg_search_topk_workspace_bytes(web, 2, 100, 5, 0) == -1
