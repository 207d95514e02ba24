"""Host side of the embed-once search API (include/siamese_search.h): the library exports
exactly the header's symbols next to the unchanged other headers' sets, sg_search_topk
checks its arguments before any HIP call, and its workspace holds nothing proportional to
m·n (so all of this runs without a GPU)."""
import ctypes
import os
import re

import pytest

from _embed_fixtures import lib_model, ntn_stack, problem
from graphembedding_amd import _lib
from graphembedding_amd.build import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM_RE = r'^\s*(?:int32_t|int64_t)\s+(sg_\w+)\s*\('   # test_lib_abi.header_symbols


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def test_search_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_search.h')
    assert set(syms) == set(_lib.SEARCH_SYMBOLS), syms
    assert len(_lib.SEARCH_SYMBOLS) == len(set(_lib.SEARCH_SYMBOLS)) == 2
    for s in syms:
        assert hasattr(L, s), s
    assert L.sg_version() == 11000


def test_search_symbols_are_disjoint_from_the_other_headers():
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EMBED_SYMBOLS, _lib.EMBED_TRAIN_SYMBOLS):
        assert not set(_lib.SEARCH_SYMBOLS) & set(other)
    for name in ('siamese_hip.h', 'siamese_embed.h', 'siamese_embed_train.h'):
        assert not set(_lib.SEARCH_SYMBOLS) & set(_header_symbols(name)), name


def _search_rc(L, m, q=1, db=1, mm=2, nn=100, prm=1, k=5, seg=0, idx=1, val=1, ws=1):
    """sg_search_topk with dummy non-null pointers: only paths that return before the first
    launch are exercised (test_embed_abi._grid_rc)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    return L.sg_search_topk(m, p if q else None, p if db else None, mm, nn, p if prm else None,
                            1, k, 1, seg, p if idx else None, p if val else None,
                            p if ws else None, None)


def test_search_refuses_what_the_grid_refuses(L):
    dot = lib_model(problem(dict(num_layers=5, layer_4='Dot')))
    k17 = lib_model(problem(ntn_stack(10, 17)))
    d32 = lib_model(problem(ntn_stack(32, 10), n_max=32, n_lo=5, n_hi=30), n_max=32)
    web = lib_model(problem(n_max=64, n_lo=5, n_hi=40), n_max=64)
    assert _lib.validate(k17)[0] > 0 and _lib.validate(web)[1] == _lib.PATH_WEB
    for name, m in (('dot', dot), ('k17', k17), ('d32', d32), ('web', web)):
        assert _search_rc(L, m) == _lib.SG_ERR_UNSUPPORTED, name
        assert L.sg_search_topk_workspace_bytes(m, 2, 100, 5, 0) == -1, name
        with pytest.raises(_lib.SiameseHipError):
            _lib.search_workspace_bytes(m, 2, 100, 5)
    assert _search_rc(L, None) == _lib.SG_ERR_ARG
    assert L.sg_search_topk_workspace_bytes(None, 2, 100, 5, 0) == -1


def test_search_host_validation(L):
    ok = lib_model(problem(ntn_stack(31, 16), n_max=31, n_lo=5, n_hi=30), n_max=32)
    for m in (ok, lib_model(problem())):
        assert _search_rc(L, m, k=0) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, k=-3) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, nn=10, k=11) == _lib.SG_ERR_ARG                # k > n
        assert _search_rc(L, m, nn=0, k=1) == _lib.SG_ERR_ARG                  # k > n = 0
        assert _search_rc(L, m, nn=100, k=65) == _lib.SG_ERR_UNSUPPORTED       # k > 64
        assert _search_rc(L, m, nn=10, k=65) == _lib.SG_ERR_UNSUPPORTED        # as sg_topk_rows
        for seg in (100, -64, 1, 63, 65):
            assert _search_rc(L, m, seg=seg) == _lib.SG_ERR_ARG, seg
            assert L.sg_search_topk_workspace_bytes(m, 2, 100, 5, seg) == -1, seg
        assert _search_rc(L, m, mm=-1) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, nn=-1) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, mm=(1 << 29) + 1) == _lib.SG_ERR_UNSUPPORTED
        assert _search_rc(L, m, nn=(1 << 29) + 1) == _lib.SG_ERR_UNSUPPORTED
        for null in ('q', 'db', 'prm', 'idx', 'ws'):
            assert _search_rc(L, m, **{null: 0}) == _lib.SG_ERR_ARG, null
        # no rows: no work, whatever the pointers; the argument checks still come first
        assert _search_rc(L, m, mm=0, q=0, idx=0, val=0, ws=0) == _lib.SG_OK
        assert _search_rc(L, m, mm=0, k=0) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, mm=0, seg=100) == _lib.SG_ERR_ARG
        for k, seg in ((0, 0), (65, 0), (101, 0), (5, 100)):
            assert L.sg_search_topk_workspace_bytes(m, 2, 100, k, seg) == -1, (k, seg)


def _q_bytes(model, m):
    """The query tables Q [m][Dp][16] of the score grid, as its own workspace query gives
    them."""
    return int(_lib.lib().sg_score_grid_workspace_bytes(model, m))


def test_search_workspace_does_not_grow_with_m_times_n(L):
    """256 queries against 2^20 database rows, k = 10, segments of 4096 columns: the tables
    plus 256 segments x 256 x 10 candidates of at most 16 B, under 12 MB where the two-call
    path needs the 1 GB matrix."""
    model = lib_model(problem())
    m, n, k, seg = 256, 1 << 20, 10, 4096
    b = L.sg_search_topk_workspace_bytes(model, m, n, k, seg)
    bound = _q_bytes(model, m) + (n // seg) * m * k * 16 + 4096
    assert 0 < b <= bound < 12 << 20 < m * n * 4 == 1 << 30, (b, bound)
    # the header's formula
    q = (m * 12 * 16 * 4 + 255) & ~255
    assert b == q + (n // seg) * m * k * 12 + 256
    # the library's own choice: sized for its shortest segments, 1024 columns
    b0 = L.sg_search_topk_workspace_bytes(model, m, n, k, 0)
    assert b0 == q + (n // 1024) * m * k * 12 + 256 < 32 << 20
    # a segment longer than the database is one segment
    assert L.sg_search_topk_workspace_bytes(model, 4, 100, 5, 1 << 40) == \
        L.sg_search_topk_workspace_bytes(model, 4, 100, 5, 128)


def test_search_workspace_is_monotone(L):
    model = lib_model(problem())
    for seg in (0, 64, 4096):
        by_m = [L.sg_search_topk_workspace_bytes(model, m, 100000, 10, seg)
                for m in (0, 1, 2, 5, 64, 1000, 100000)]
        by_k = [L.sg_search_topk_workspace_bytes(model, 64, 100000, k, seg)
                for k in (1, 2, 10, 63, 64)]
        assert by_m[0] >= 0 and by_m == sorted(by_m) and len(set(by_m)) == len(by_m), by_m
        assert by_k[0] > 0 and by_k == sorted(by_k) and len(set(by_k)) == len(by_k), by_k
