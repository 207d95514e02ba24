"""Host side of embed-once training with graph-keyed dropout (include/siamese_embed_drop.h):
the library exports exactly the header's symbols, every refusal the header lists is returned
before any HIP call (dummy pointers, no GPU), the backward's workspace is sg_embed_bwd's, and
the older calls keep their refusals."""
import ctypes
import os
import re

import pytest

from _embed_fixtures import lib_model, ntn_stack, problem
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


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _fwd_rc(L, m, n_graphs=4, n_max=10, count=2, entry_offset=0, seed=7, **null):
    """sg_embed_drop with dummy non-null pointers (null=0 nulls one): only paths that return
    before the first launch are exercised."""
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_embed_drop(m, p('adj'), p('types'), p('n'), n_graphs, n_max, None, count,
                           entry_offset, p('prm'), seed, p('out'), None, None)


def _bwd_rc(L, m, n_graphs=4, n_max=10, count=2, entry_offset=0, seed=7, **null):
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_embed_drop_bwd(m, p('adj'), p('types'), p('n'), n_graphs, n_max, None, count,
                               entry_offset, p('prm'), seed, p('gemb'), p('grad'), None, p('ws'),
                               None)


def test_drop_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_embed_drop.h')
    assert set(syms) == set(_lib.EMBED_DROP_SYMBOLS), syms
    assert len(_lib.EMBED_DROP_SYMBOLS) == len(set(_lib.EMBED_DROP_SYMBOLS)) == 3
    for s in syms:
        assert hasattr(L, s), s
    for other in (_lib.EXPORTED_SYMBOLS, _lib.EMBED_SYMBOLS, _lib.EMBED_TRAIN_SYMBOLS,
                  _lib.SEARCH_SYMBOLS):
        assert not set(_lib.EMBED_DROP_SYMBOLS) & set(other)
    # the older headers keep their symbol sets; the new symbols are the feature test
    assert set(_lib.EXPORTED_SYMBOLS) == set(_header_symbols('siamese_hip.h'))
    assert set(_lib.EMBED_SYMBOLS) == set(_header_symbols('siamese_embed.h'))
    assert set(_lib.EMBED_TRAIN_SYMBOLS) == set(_header_symbols('siamese_embed_train.h'))
    assert set(_lib.SEARCH_SYMBOLS) == set(_header_symbols('siamese_search.h'))
    assert L.sg_version() == 11000
    text = open(os.path.join(ROOT, 'include', 'siamese_embed_drop.h')).read()
    assert 'presence of the symbols' in text
    assert 'layers.py:334-336' in text and 'A4' in text   # the lines it deviates from


def test_host_refusals_before_any_hip_call(L):
    """The header's table, for both calls, with a dropped model (keep 0.9, the default
    stack's dropout=True layers) the calls are made for."""
    prob = problem()
    m = lib_model(prob, keep_prob=0.9)
    for rc in (_fwd_rc, _bwd_rc):
        assert rc(L, None) == _lib.SG_ERR_ARG                                  # NULL model
        assert rc(L, m, count=-1) == _lib.SG_ERR_ARG
        assert rc(L, m, entry_offset=-2) == _lib.SG_ERR_ARG
        assert rc(L, m, entry_offset=1) == _lib.SG_ERR_ARG                     # odd
        assert rc(L, m, entry_offset=7, count=0) == _lib.SG_ERR_ARG            # before the count
        for keep in (0.0, -0.5, 1.5, float('nan')):
            assert rc(L, lib_model(prob, keep_prob=keep)) == _lib.SG_ERR_ARG, keep
        assert rc(L, m, n_graphs=0) == _lib.SG_ERR_ARG
        assert rc(L, m, n_max=12) == _lib.SG_ERR_ARG                           # the store's slots
    # path 3 (graph store), at any keep_prob
    for keep in (0.9, 1.0):
        web = lib_model(problem(None, n_max=64, n_lo=5, n_hi=40), n_max=64, keep_prob=keep)
        assert _lib.validate(web)[1] == _lib.PATH_WEB
        assert _fwd_rc(L, web, n_max=64) == _lib.SG_ERR_UNSUPPORTED
        assert _bwd_rc(L, web, n_max=64) == _lib.SG_ERR_UNSUPPORTED
        assert L.sg_embed_drop_bwd_workspace_bytes(web, 4) == -1
    # a stack that does not fit the LDS, as sg_embed refuses it: one wavefront's slice of
    # the generic layout above 160 KB (GCN widths 256 at capacity 60, off path 3)
    wide = dict(layer_0='GraphConvolution:output_dim=256,dropout=True,bias=True,act=relu,'
                        'sparse_inputs=True',
                layer_1='GraphConvolution:input_dim=256,output_dim=256,dropout=True,bias=True,'
                        'act=identity,sparse_inputs=False',
                layer_2='Dense:input_dim=256,output_dim=1,dropout=True,bias=True,act=relu',
                layer_3='Padding:max_in_dims=30,padding_value=0',
                layer_4='NTN:input_dim=30,feature_map_dim=10,inneract=relu,dropout=True,'
                        'bias=True')
    big = lib_model(problem(wide, n_max=30, n_lo=5, n_hi=30), n_max=60, keep_prob=0.9)
    plain =lib_model(problem(dict(wide, dropout=0.0), n_max=30, n_lo=5, n_hi=30), n_max=60)
    assert L.sg_embed(plain, _P, _P, _P, 4, 60, None, 2, _P, _P, None, None) == \
        _lib.SG_ERR_UNSUPPORTED
    assert _fwd_rc(L, big, n_max=60) == _lib.SG_ERR_UNSUPPORTED
    assert _bwd_rc(L, big, n_max=60) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_embed_drop_bwd_workspace_bytes(big, 4) == -1
    # accepted models: the next checks are the pointers', still on the host
    assert _fwd_rc(L, m, count=0, adj=0, out=0) == _lib.SG_OK                  # nothing to do
    for name in ('adj', 'types', 'n', 'prm', 'out'):
        assert _fwd_rc(L, m, **{name: 0}) == _lib.SG_ERR_ARG, name
    for name in ('adj', 'types', 'n', 'prm', 'gemb', 'grad', 'ws'):
        assert _bwd_rc(L, m, entry_offset=4, **{name: 0}) == _lib.SG_ERR_ARG, name


def test_bwd_workspace_is_embed_bwd_workspace(L):
    prob = problem()
    stacks = [prob, problem(dict(AVERAGE_STACK)), problem(ntn_stack(10, 16))]
    for pr in stacks:
        plain = lib_model(pr, keep_prob=1.0)
        dropped = lib_model(pr, keep_prob=0.9)
        for count in (0, 1, 2, 7, 700, 100_000):
            want = L.sg_embed_bwd_workspace_bytes(plain, count)
            assert want > 0
            assert L.sg_embed_drop_bwd_workspace_bytes(plain, count) == want
            # dropout changes no shape: the dropped model needs the same bytes
            assert L.sg_embed_drop_bwd_workspace_bytes(dropped, count) == want
    m = lib_model(prob, keep_prob=0.9)
    assert L.sg_embed_drop_bwd_workspace_bytes(m, -1) == -1
    assert L.sg_embed_drop_bwd_workspace_bytes(None, 4) == -1
    assert L.sg_embed_drop_bwd_workspace_bytes(lib_model(prob, keep_prob=0.0), 4) == -1
    with pytest.raises(_lib.SiameseHipError, match='graph-keyed'):
        _lib.embed_drop_bwd_workspace_bytes(lib_model(prob, keep_prob=0.0), 4)


def test_older_calls_keep_their_refusals(L):
    dropped = lib_model(problem(), keep_prob=0.9)
    assert L.sg_embed_bwd(dropped, _P, _P, _P, 4, 10, None, 2, _P, _P, _P, None, _P, None) == \
        _lib.SG_ERR_UNSUPPORTED
    assert L.sg_embed_bwd_workspace_bytes(dropped, 4) == -1
    assert L.sg_score_grid_bwd_workspace_bytes(dropped, 4, 4) == -1
    assert L.sg_topk_rows(_P, 1, 100, 100, 65, 1, _P, _P, None) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_topk_rows(_P, 1, 100, 100, 0, 1, _P, _P, None) == _lib.SG_ERR_ARG
