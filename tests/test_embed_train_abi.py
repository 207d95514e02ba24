"""Host side of the embed-once training API (include/siamese_embed_train.h): the library
exports exactly the header's symbols next to the two older, unchanged sets, and both calls
check their arguments and refuse dropout, path 3 and heads the grid does not serve before
any HIP call (so all of this runs without a GPU)."""
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


def test_train_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_embed_train.h')
    assert set(syms) == set(_lib.EMBED_TRAIN_SYMBOLS), syms
    assert len(_lib.EMBED_TRAIN_SYMBOLS) == len(set(_lib.EMBED_TRAIN_SYMBOLS)) == 4
    for s in syms:
        assert hasattr(L, s), s
    assert not set(_lib.EMBED_TRAIN_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    assert not set(_lib.EMBED_TRAIN_SYMBOLS) & set(_lib.EMBED_SYMBOLS)
    # the older headers keep their symbol sets; the new symbols are the feature test
    assert set(_lib.EXPORTED_SYMBOLS) == set(_header_symbols('siamese_hip.h'))
    assert set(_lib.EMBED_SYMBOLS) == set(_header_symbols('siamese_embed.h'))
    assert L.sg_version() == 11000
    assert 'presence of the symbols' in open(os.path.join(
        ROOT, 'include', 'siamese_embed_train.h')).read()


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _grid_rc(L, m, mm=1, nn=1, ld_lab=None, ld_s=None, batch_total=1, **null):
    """sg_score_grid_fwd_bwd with dummy non-null pointers (null=0 nulls one): only paths
    that return before the first launch are exercised."""
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_score_grid_fwd_bwd(m, p('q'), p('db'), mm, nn, p('prm'), p('lab'),
                                   nn if ld_lab is None else ld_lab, batch_total, p('ys'), 1,
                                   p('s'), nn if ld_s is None else ld_s, p('gq'), p('gdb'),
                                   p('grad'), p('loss'), p('ws'), None)


def _embed_rc(L, m, n_graphs=4, n_max=10, count=2, **null):
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_embed_bwd(m, p('adj'), p('types'), p('n'), n_graphs, n_max, None, count,
                          p('prm'), p('gemb'), p('grad'), None, p('ws'), None)


def _no_dropout_layers(prob):
    return [dict(Ly, dropout=False) for Ly in prob.layers]


def test_grid_fwd_bwd_host_validation(L):
    ok = lib_model(problem(ntn_stack(31, 16, dropout=0.0), n_max=31, n_lo=5, n_hi=30), n_max=32)
    assert _grid_rc(L, None) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, mm=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, nn=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, ok, mm=2, nn=3, ld_lab=2) == _lib.SG_ERR_ARG          # ld_labels < n
    assert _grid_rc(L, ok, mm=2, nn=3, ld_s=2) == _lib.SG_ERR_ARG            # ld_s < n
    for name in ('q', 'db', 'prm', 'gq', 'gdb', 'grad', 'ws', 'ys'):         # broadcast: y_stats
        assert _grid_rc(L, ok, mm=2, nn=3, **{name: 0}) == _lib.SG_ERR_ARG, name
    # empty grids: no work, whatever the pointers
    assert _grid_rc(L, ok, mm=0, q=0, gq=0, ws=0) == _lib.SG_OK
    assert _grid_rc(L, ok, nn=0, db=0, gdb=0, ws=0) == _lib.SG_OK
    # the aligned loss needs labels and a batch size instead of y_stats
    al = lib_model(problem(ntn_stack(10, 10, dropout=0.0, loss_mode='aligned')))
    assert _grid_rc(L, al, mm=2, nn=3, lab=0) == _lib.SG_ERR_ARG
    assert _grid_rc(L, al, mm=2, nn=3, batch_total=0) == _lib.SG_ERR_ARG
    assert L.sg_score_grid_bwd_workspace_bytes(ok, 3, 5) >= (3 + 3 + 3) * 32 * 16 * 4
    assert L.sg_score_grid_bwd_workspace_bytes(ok, -1, 5) == -1
    assert L.sg_score_grid_bwd_workspace_bytes(ok, 3, (1 << 29) + 1) == -1
    assert L.sg_score_grid_bwd_workspace_bytes(None, 3, 5) == -1
    # the partials of 2^23 column blocks x 2^29 queries do not fit an int64 of bytes
    assert L.sg_score_grid_bwd_workspace_bytes(ok, 1 << 29, 1 << 29) == -1


# (D, K, m, n): bytes, as the library returned them when the grid call was first merged.  The
# call is host arithmetic, independent of the device: the literals pin the query-chunk split
# (1024 workgroups aimed for) and the workspace layout.
GRID_BWD_WORKSPACE_BYTES = {
    (10, 10, 1, 1): 7936,
    (10, 10, 37, 200): 260864,
    (31, 16, 5, 65): 123392,
    (16, 1, 4, 64): 21248,
    (10, 10, 700, 700): 9630208,
    (11, 10, 4097, 63): 11302144,
}


def test_grid_bwd_workspace_bytes_are_pinned(L):
    for (D, K, m, n), want in GRID_BWD_WORKSPACE_BYTES.items():
        if D == 10:
            model = lib_model(problem(ntn_stack(D, K, dropout=0.0)))
        elif D == 31:   # Padding(31) on the capacity-32 records
            model = lib_model(problem(ntn_stack(D, K, dropout=0.0), n_max=31, n_lo=5, n_hi=30),
                              n_max=32)
        else:
            model = lib_model(problem(ntn_stack(D, K, dropout=0.0), n_max=D), n_max=D)
        assert L.sg_score_grid_bwd_workspace_bytes(model, m, n) == want, (D, K, m, n)


def test_both_calls_refuse_dropout(L):
    """keep_prob = 0.9 with the default stack's dropout=True layers: refused; the same
    stack and keep_prob with every layer's dropout=False has no effective dropout."""
    prob = problem()
    dropped = lib_model(prob, keep_prob=0.9)
    assert _lib.validate(dropped)[0] > 0
    assert _grid_rc(L, dropped) == _lib.SG_ERR_UNSUPPORTED
    assert _grid_rc(L, dropped, mm=0) == _lib.SG_ERR_UNSUPPORTED             # before the counts
    assert _embed_rc(L, dropped) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_score_grid_bwd_workspace_bytes(dropped, 4, 4) == -1
    assert L.sg_embed_bwd_workspace_bytes(dropped, 4) == -1
    f = prob.flags
    plain = _lib.make_model(_no_dropout_layers(prob), prob.d_in, prob.n_max, 0.9, f.final_act,
                            f.sim_kernel, f.yeta, f.loss_mode, f.ntn_mode)
    assert _grid_rc(L, plain, mm=0) == _lib.SG_OK
    assert L.sg_score_grid_bwd_workspace_bytes(plain, 4, 4) > 0
    assert L.sg_embed_bwd_workspace_bytes(plain, 4) > 0
    assert _embed_rc(L, plain, ws=0) == _lib.SG_ERR_ARG                      # accepted: next check
    # only the head drops
    head_only = _no_dropout_layers(prob)
    head_only[-1]['dropout'] = True
    hm = _lib.make_model(head_only, prob.d_in, prob.n_max, 0.9, f.final_act, f.sim_kernel,
                         f.yeta, f.loss_mode, f.ntn_mode)
    assert _grid_rc(L, hm) == _lib.SG_ERR_UNSUPPORTED
    assert _embed_rc(L, hm) == _lib.SG_ERR_UNSUPPORTED
    # keep_prob = 1 is what flags.dropout = 0 builds
    assert L.sg_embed_bwd_workspace_bytes(lib_model(prob, keep_prob=1.0), 4) > 0


def test_both_calls_refuse_unserved_models(L):
    web = lib_model(problem(dict(dropout=0.0), n_max=64, n_lo=5, n_hi=40), n_max=64)
    assert _lib.validate(web)[1] == _lib.PATH_WEB
    assert _grid_rc(L, web) == _lib.SG_ERR_UNSUPPORTED
    assert _embed_rc(L, web, n_max=64) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_score_grid_bwd_workspace_bytes(web, 4, 4) == -1
    assert L.sg_embed_bwd_workspace_bytes(web, 4) == -1
    assert L.sg_embed_dim(web) == -1
    dot = lib_model(problem(dict(num_layers=5, layer_4='Dot', dropout=0.0)))
    k17 = lib_model(problem(ntn_stack(10, 17, dropout=0.0)))
    d32 = lib_model(problem(ntn_stack(32, 10, dropout=0.0), n_max=32, n_lo=5, n_hi=30), n_max=32)
    for m in (dot, k17, d32):
        assert _lib.validate(m)[0] > 0
        assert _grid_rc(L, m) == _lib.SG_ERR_UNSUPPORTED
        assert L.sg_score_grid_bwd_workspace_bytes(m, 4, 4) == -1
    # the node-stack backward has no head: the Dot and the K = 17 models are served
    assert L.sg_embed_bwd_workspace_bytes(dot, 4) > 0
    assert L.sg_embed_bwd_workspace_bytes(k17, 4) > 0


def test_embed_bwd_host_validation(L):
    m = lib_model(problem(dict(dropout=0.0)))
    assert _embed_rc(L, None) == _lib.SG_ERR_ARG
    assert _embed_rc(L, m, count=-1) == _lib.SG_ERR_ARG
    assert _embed_rc(L, m, n_graphs=0) == _lib.SG_ERR_ARG
    assert _embed_rc(L, m, n_max=12) == _lib.SG_ERR_ARG                      # the store's slots
    for name in ('adj', 'types', 'n', 'prm', 'gemb', 'grad', 'ws'):
        assert _embed_rc(L, m, **{name: 0}) == _lib.SG_ERR_ARG, name
    assert L.sg_embed_bwd_workspace_bytes(m, -1) == -1
    assert L.sg_embed_bwd_workspace_bytes(None, 4) == -1
    avg = lib_model(problem(dict(AVERAGE_STACK, dropout=0.0)))
    assert L.sg_embed_bwd_workspace_bytes(avg, 7) > 0


def test_python_wrappers_name_the_reason(L):
    dropped = lib_model(problem(), keep_prob=0.9)
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        _lib.score_grid_bwd_workspace_bytes(dropped, 4, 4)
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        _lib.embed_bwd_workspace_bytes(dropped, 4)
