"""Host side of the embed-once retrieval API (include/siamese_embed.h): the library
exports exactly the header's symbols next to the unchanged siamese_hip.h set, sg_embed_dim
reads the head's per-graph width off the plan, and sg_score_grid / sg_topk_rows check their
arguments before any HIP call (so all of this runs without a GPU)."""
import json
import os
import re
import sys

import pytest

from _embed_fixtures import ATTENTION_STACK, lib_model, ntn_stack, problem
from _fixtures import AVERAGE_STACK
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


def test_embed_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_embed.h')
    assert set(syms) == set(_lib.EMBED_SYMBOLS), syms
    assert len(_lib.EMBED_SYMBOLS) == len(set(_lib.EMBED_SYMBOLS)) == 5
    for s in syms:
        assert hasattr(L, s), s
    assert L.sg_version() == 11000


def test_exported_symbols_unchanged(L):
    assert set(_lib.EXPORTED_SYMBOLS) == set(_header_symbols('siamese_hip.h'))
    assert len(_lib.EXPORTED_SYMBOLS) == 36
    assert not set(_lib.EXPORTED_SYMBOLS) & set(_lib.EMBED_SYMBOLS)


def test_embed_dim(L):
    assert _lib.embed_dim(lib_model(problem())) == 10                 # Padding 10 x Dense 1
    c4 = problem(n_max=30, n_lo=5, n_hi=30)
    assert _lib.embed_dim(lib_model(c4, n_max=32)) == 30              # Padding 30 at capacity 32
    assert _lib.embed_dim(lib_model(problem(AVERAGE_STACK))) == 16    # GCN width
    assert _lib.embed_dim(lib_model(problem(ATTENTION_STACK))) == 16
    web = problem(n_max=64, n_lo=5, n_hi=40)                          # path 3: out of scope
    m = lib_model(web, n_max=64)
    assert _lib.validate(m)[1] == _lib.PATH_WEB
    assert L.sg_embed_dim(m) == -1
    with pytest.raises(_lib.SiameseHipError):
        _lib.embed_dim(m)
    bad = lib_model(problem())
    bad.num_layers = 1
    assert L.sg_embed_dim(bad) == -1
    assert L.sg_embed_dim(None) == -1


def test_embed_dim_ignores_keep_prob(L):
    m = lib_model(problem(), keep_prob=0.9)
    m.keep_prob = 0.0          # invalid for training; the inference calls read it as 1
    assert L.sg_embed_dim(m) == 10


def _grid_rc(L, m, q=1, db=1, mm=1, nn=1, prm=1, out=1, ld=None, ws=1):
    """sg_score_grid with dummy non-null pointers: only paths that return before the first
    launch are exercised."""
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    return L.sg_score_grid(m, p if q else None, p if db else None, mm, nn, p if prm else None,
                           0, p if out else None, nn if ld is None else ld, p if ws else None,
                           None)


def test_score_grid_host_validation(L):
    dot = lib_model(problem(dict(num_layers=5, layer_4='Dot')))
    assert _grid_rc(L, dot) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_score_grid_workspace_bytes(dot, 4) == -1
    k17 = lib_model(problem(ntn_stack(10, 17)))
    assert _lib.validate(k17)[0] > 0                                   # a valid model ...
    assert _grid_rc(L, k17) == _lib.SG_ERR_UNSUPPORTED                 # ... above one k tile
    d32 = lib_model(problem(ntn_stack(32, 10), n_max=32, n_lo=5, n_hi=30), n_max=32)
    assert _grid_rc(L, d32) == _lib.SG_ERR_UNSUPPORTED
    ok = lib_model(problem(ntn_stack(31, 16), n_max=31, n_lo=5, n_hi=30), n_max=32)
    assert L.sg_score_grid_workspace_bytes(ok, 3) >= 3 * 32 * 16 * 4   # Q[m][Dp = 32][16]
    assert L.sg_score_grid_workspace_bytes(lib_model(problem()), 3) >= 3 * 12 * 16 * 4
    for null in ('q', 'db', 'prm', 'out', 'ws'):
        assert _grid_rc(L, ok, mm=2, nn=3, **{null: 0}) == _lib.SG_ERR_ARG, null
    assert _grid_rc(L, ok, mm=2, nn=3, ld=2) == _lib.SG_ERR_ARG        # ld_out < n
    assert _grid_rc(L, ok, mm=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, None) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, mm=0, q=0, out=0) == _lib.SG_OK             # empty grid: no work


def test_embed_host_validation(L):
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    m = lib_model(problem())
    assert L.sg_embed(m, p, p, p, 4, 10, None, 0, p, p, None, None) == _lib.SG_OK
    assert L.sg_embed(m, p, p, p, 4, 12, None, 2, p, p, None, None) == _lib.SG_ERR_ARG   # n_max
    assert L.sg_embed(m, None, p, p, 4, 10, None, 2, p, p, None, None) == _lib.SG_ERR_ARG
    assert L.sg_embed(m, p, p, p, 4, 10, None, 2, p, None, None, None) == _lib.SG_ERR_ARG
    assert L.sg_embed(m, p, p, p, 0, 10, None, 2, p, p, None, None) == _lib.SG_ERR_ARG
    assert L.sg_embed(m, p, p, p, 4, 10, None, -1, p, p, None, None) == _lib.SG_ERR_ARG
    web = lib_model(problem(n_max=64, n_lo=5, n_hi=40), n_max=64)
    assert L.sg_embed(web, p, p, p, 4, 64, None, 2, p, p, None, None) == _lib.SG_ERR_UNSUPPORTED


def test_topk_host_validation(L):
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert L.sg_topk_rows(p, 1, 100, 100, 0, 1, p, p, None) == _lib.SG_ERR_ARG          # k = 0
    assert L.sg_topk_rows(p, 1, 10, 10, 11, 1, p, p, None) == _lib.SG_ERR_ARG           # k > n
    assert L.sg_topk_rows(p, 1, 100, 100, 65, 1, p, p, None) == _lib.SG_ERR_UNSUPPORTED  # k > 64
    assert L.sg_topk_rows(p, 1, 100, 99, 5, 1, p, p, None) == _lib.SG_ERR_ARG           # ld < n
    assert L.sg_topk_rows(None, 1, 100, 100, 5, 1, p, p, None) == _lib.SG_ERR_ARG
    assert L.sg_topk_rows(p, 1, 100, 100, 5, 1, None, p, None) == _lib.SG_ERR_ARG
    assert L.sg_topk_rows(p, 0, 100, 100, 5, 1, p, None, None) == _lib.SG_OK            # no rows


def test_test_path_flag_defaults_to_pairs():
    from graphembedding_amd.config import Flags
    assert Flags().test_path == 'pairs'


def test_fused_kernel_sources_untouched():
    """The retrieval work leaves the hashed fused-kernel sources byte-identical, so the
    bench line keeps the PMC traffic of profiles/traffic.json."""
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, 'profiles', 'traffic.json')) as f:
        assert bench.fused_kernel_source_hash() == json.load(f)['sources_sha1']
