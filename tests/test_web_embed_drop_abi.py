"""Host side of embed-once training with graph-keyed dropout for graph-store (Web) models
(include/siamese_web_embed_drop.h): the library exports exactly the header's symbols next to
the unchanged other headers, every refusal the header lists is returned before any HIP call
(dummy pointers, so all of this runs without a GPU), the workspace queries follow the header's
formulas, and the older Web training calls keep their dropout refusal."""
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
                 'siamese_web_search.h': 'WEB_SEARCH_SYMBOLS',
                 'siamese_web_embed_train.h': 'WEB_EMBED_TRAIN_SYMBOLS'}
MAX_ROWS = 1 << 29


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def _web(D, K=10, keep_prob=0.9, **kw):
    """A path-3 model of Padding / NTN width D with every layer's dropout flag set."""
    prob = problem(ntn_stack(D, K, **kw), n_max=D, n_lo=5, n_hi=min(D, 40))
    return lib_model(prob, n_max=D, keep_prob=keep_prob)


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _store(n_graphs=4, n_max=40, **null):
    s = _lib.SgCsrStore()
    s.n_graphs, s.n_max, s.max_nnz = n_graphs, n_max, 8
    for f in ('node_off', 'types', 'row_ptr', 'col', 'val'):
        setattr(s, f, None if null.get(f) == 0 else _P)
    return s


def _fwd_rc(L, m, store, count=2, entry_offset=0, seed=7, ld_g=None, **null):
    """sg_web_embed_drop with dummy non-null pointers (name=0 passes NULL): only paths that
    return before the first launch are exercised.  (ld_g: ignored, so both calls share the
    table below.)"""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_web_embed_drop(m, store, None, count, entry_offset, p('prm'), seed, p('out'),
                               None, p('ws'), None)


def _bwd_rc(L, m, store, count=2, entry_offset=0, seed=7, ld_g=64, **null):
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    return L.sg_web_embed_drop_bwd(m, store, None, count, entry_offset, p('prm'), seed, p('g'),
                                   ld_g, p('grad'), None, p('ws'), None)


def test_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_web_embed_drop.h')
    assert set(syms) == set(_lib.WEB_EMBED_DROP_SYMBOLS), syms
    # the three calls of the contract and the forward's workspace query (its side-major
    # staging does not fit sg_web_embed's workspace)
    assert len(_lib.WEB_EMBED_DROP_SYMBOLS) == len(set(_lib.WEB_EMBED_DROP_SYMBOLS)) == 4
    for s in ('sg_web_embed_drop', 'sg_web_embed_drop_bwd_workspace_bytes',
              'sg_web_embed_drop_bwd', 'sg_web_embed_drop_workspace_bytes'):
        assert s in syms and hasattr(L, s), s
    for fn in ('web_embed_drop', 'web_embed_drop_bwd_workspace_bytes', 'web_embed_drop_bwd',
               'web_embed_drop_workspace_bytes'):
        assert callable(getattr(_lib, fn)), fn
    assert L.sg_version() == 11000
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.WEB_EMBED_DROP_SYMBOLS) & set(other), name
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged
    text = open(os.path.join(ROOT, 'include', 'siamese_web_embed_drop.h')).read()
    assert 'presence of the symbols' in text
    assert 'layers.py:334-336' in text and 'A4' in text   # the lines it deviates from


def test_host_refusals_before_any_hip_call(L):
    """The header's table, for both calls, with a dropped model (keep 0.9, every layer's
    dropout flag set): the model the calls are made for."""
    m = _web(64)
    st = _store()
    assert _lib.validate(m)[1] == _lib.PATH_WEB
    for rc in (_fwd_rc, _bwd_rc):
        assert rc(L, None, st) == _lib.SG_ERR_ARG                              # NULL model
        assert rc(L, m, st, count=-1) == _lib.SG_ERR_ARG
        assert rc(L, m, st, entry_offset=-2) == _lib.SG_ERR_ARG
        assert rc(L, m, st, entry_offset=1) == _lib.SG_ERR_ARG                 # odd
        assert rc(L, m, st, entry_offset=7, count=0) == _lib.SG_ERR_ARG        # before the count
        for keep in (0.0, -0.5, 1.5, float('nan')):
            assert rc(L, _web(64, keep_prob=keep), st) == _lib.SG_ERR_ARG, keep
        # models off path 3: the default stack (path 1), capacity 32 (path 2), the Dot head
        for other in (lib_model(problem()),
                      lib_model(problem(n_max=30, n_lo=5, n_hi=30), n_max=32),
                      lib_model(problem(dict(num_layers=5, layer_4='Dot')))):
            assert _lib.validate(other)[1] != _lib.PATH_WEB
            assert rc(L, other, st) == _lib.SG_ERR_UNSUPPORTED
        assert rc(L, _web(64, 17), st) == _lib.SG_ERR_UNSUPPORTED              # K above 16
        # a bad store
        assert rc(L, m, None) == _lib.SG_ERR_ARG
        for f in ('node_off', 'types', 'row_ptr', 'col', 'val'):
            assert rc(L, m, _store(**{f: 0})) == _lib.SG_ERR_ARG, f
        assert rc(L, m, _store(n_max=65)) == _lib.SG_ERR_ARG                   # store n_max > D
        assert rc(L, m, _store(n_max=0)) == _lib.SG_ERR_ARG
        assert rc(L, m, _store(n_graphs=-1)) == _lib.SG_ERR_ARG
        # entry numbers stay below 2^29
        assert rc(L, m, st, count=MAX_ROWS + 1) == _lib.SG_ERR_UNSUPPORTED
        assert rc(L, m, st, count=2, entry_offset=MAX_ROWS) == _lib.SG_ERR_UNSUPPORTED
        assert rc(L, m, st, count=MAX_ROWS, entry_offset=2) == _lib.SG_ERR_UNSUPPORTED
        # accepted so far: the pointers, still on the host
        assert rc(L, m, st, prm=0) == _lib.SG_ERR_ARG
        assert rc(L, m, st, ws=0) == _lib.SG_ERR_ARG
        assert rc(L, m, st, entry_offset=4, ws=0) == _lib.SG_ERR_ARG
    assert _fwd_rc(L, m, st, out=0) == _lib.SG_ERR_ARG
    assert _fwd_rc(L, m, st, count=0, out=0, prm=0, ws=0) == _lib.SG_OK        # nothing to do
    for null in ('g', 'grad'):
        assert _bwd_rc(L, m, st, **{null: 0}) == _lib.SG_ERR_ARG, null
    assert _bwd_rc(L, m, st, count=0, grad=0) == _lib.SG_ERR_ARG               # the range to zero
    assert _bwd_rc(L, m, st, ld_g=63) == _lib.SG_ERR_ARG                       # ld_g < D
    assert _bwd_rc(L, _web(50), st, ld_g=49) == _lib.SG_ERR_ARG
    # keep_prob 1 and a stack without dropout flags are served too (bitwise sg_web_embed's):
    # they get as far as the pointer checks
    assert _fwd_rc(L, _web(64, keep_prob=1.0), st, out=0) == _lib.SG_ERR_ARG
    assert _bwd_rc(L, _web(64, keep_prob=1.0), st, ld_g=63) == _lib.SG_ERR_ARG


def _up64(x):
    return (x + 63) & ~63


def test_workspace_queries(L):
    """-1 where the calls refuse, monotone in count, and the header's formulas."""
    m = _web(64)
    for q in (L.sg_web_embed_drop_workspace_bytes, L.sg_web_embed_drop_bwd_workspace_bytes):
        assert q(None, 4) == -1
        assert q(m, -1) == -1
        assert q(m, MAX_ROWS + 1) == -1
        assert q(_web(64, keep_prob=0.0), 4) == -1
        assert q(_web(64, 17), 4) == -1
        assert q(lib_model(problem()), 4) == -1                                # off path 3
        for D, K in ((64, 10), (50, 1), (512, 16)):
            prev = 0
            for count in (0, 1, 2, 5, 7, 300, 1023, 1024, 1025, 1027, 100000):
                b = q(_web(D, K), count)
                assert b > 0 and b >= prev, (D, count)
                prev = b
    with pytest.raises(_lib.SiameseHipError, match='graph-keyed'):
        _lib.web_embed_drop_bwd_workspace_bytes(lib_model(problem()), 4)
    with pytest.raises(_lib.SiameseHipError, match='graph-keyed'):
        _lib.web_embed_drop_workspace_bytes(lib_model(problem()), 4)
    for D in (50, 64, 512):
        model, plain = _web(D, 16), _web(D, 16, keep_prob=1.0)
        Dp = L.sg_web_embed_ld(model)
        assert Dp == (D + 127) // 128 * 128
        n_gcn = model.d_in * 32 + 32 + 32 * 16 + 16 + 16 + 1   # W0 b0 W1 b1 Wd bd
        for count in (1, 2, 5, 67, 1023, 1024, 1027, 5000):
            ce = (count + 1) // 2 * 2
            assert L.sg_web_embed_drop_workspace_bytes(model, count) == \
                4 * _up64(ce * Dp) + L.sg_web_embed_workspace_bytes(model, count)
            cc = min(count, 1024)
            ce = (cc + 1) // 2 * 2
            want = 4 * (_up64(512 * n_gcn) + 2 * _up64(ce * Dp) + _up64(cc * Dp * 4) +
                        _up64(cc * Dp * 32) + _up64(cc) +
                        L.sg_web_embed_workspace_bytes(model, cc) // 4) + 256
            assert L.sg_web_embed_drop_bwd_workspace_bytes(model, count) == want, (D, count)
            # dropout changes no shape; an even chunk needs what sg_web_embed_bwd needs
            assert L.sg_web_embed_drop_bwd_workspace_bytes(plain, count) == want
            if cc % 2 == 0:
                assert L.sg_web_embed_bwd_workspace_bytes(plain, count) == want
    # chunks of 1,024 entries: the backward's workspace stops growing
    assert L.sg_web_embed_drop_bwd_workspace_bytes(m, 1024) == \
        L.sg_web_embed_drop_bwd_workspace_bytes(m, 10 ** 6)


def test_older_web_calls_keep_their_refusals(L):
    dropped = _web(64, 16)
    st = _store()
    assert L.sg_web_embed_bwd(dropped, st, None, 2, _P, _P, 64, _P, None, _P, None) == \
        _lib.SG_ERR_UNSUPPORTED
    assert L.sg_web_embed_bwd_workspace_bytes(dropped, 4) == -1
    assert L.sg_web_score_grid_bwd_workspace_bytes(dropped, 4, 4) == -1
    # the small-D dropout calls keep refusing graph-store models
    assert L.sg_embed_drop_bwd_workspace_bytes(dropped, 4) == -1
    assert L.sg_embed_drop(dropped, _P, _P, _P, 4, 64, None, 2, 0, _P, 7, _P, None, None) == \
        _lib.SG_ERR_UNSUPPORTED
