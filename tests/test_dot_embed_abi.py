"""Host side of the Dot-head embed-once API (include/siamese_dot_embed.h): the library exports
exactly the header's symbols next to the older, unchanged sets; every call checks its arguments
in the header's order and refuses the NTN head, path 3, E > 512 and (the training call only)
dropout before any HIP call, so all of this runs without a GPU.  The older grid calls keep
refusing the Dot head."""
import ctypes
import os
import re

import pytest

from _embed_fixtures import lib_model, problem, sized_problem
from graphembedding_amd import _lib
from graphembedding_amd.build import build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM_RE = r'^\s*(?:int32_t|int64_t)\s+(sg_\w+)\s*\('   # test_lib_abi.header_symbols

GCN = 'GraphConvolution:{}output_dim={},act={},dropout=True,bias=True,sparse_inputs={}'


def dot_pad_stack(rows, width, **flags):
    """sparse GCN -> GCN(width) -> Padding(rows) -> Dot: E = rows * width."""
    ov = dict(num_layers=4, layer_0=GCN.format('', 8, 'relu', True),
              layer_1=GCN.format('input_dim=8,', width, 'identity', False),
              layer_2='Padding:max_in_dims={},padding_value=0'.format(rows), layer_3='Dot')
    ov.update(flags)
    return ov


def dot_model(rows=2, width=3, keep_prob=None, **flags):
    flags.setdefault('dropout', 0.0)
    prob = sized_problem([1, min(rows, 2), min(rows, 5)], dot_pad_stack(rows, width, **flags), n_max=rows)
    return lib_model(prob, keep_prob=keep_prob)


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def test_dot_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_dot_embed.h')
    assert set(syms) == set(_lib.DOT_EMBED_SYMBOLS), syms
    assert len(_lib.DOT_EMBED_SYMBOLS) == len(set(_lib.DOT_EMBED_SYMBOLS)) == 5
    for s in syms:
        assert hasattr(L, s), s
    older = (_lib.EXPORTED_SYMBOLS, _lib.EMBED_SYMBOLS, _lib.EMBED_TRAIN_SYMBOLS,
             _lib.EMBED_DROP_SYMBOLS, _lib.SEARCH_SYMBOLS, _lib.WEB_EMBED_SYMBOLS,
             _lib.WEB_SEARCH_SYMBOLS, _lib.WEB_EMBED_TRAIN_SYMBOLS, _lib.WEB_EMBED_DROP_SYMBOLS,
             _lib.EVAL_SYMBOLS)
    for group in older:
        assert not set(_lib.DOT_EMBED_SYMBOLS) & set(group)
    # the older headers keep their symbol sets; the new symbols are the feature test
    assert set(_lib.EXPORTED_SYMBOLS) == set(_header_symbols('siamese_hip.h'))
    assert set(_lib.EMBED_SYMBOLS) == set(_header_symbols('siamese_embed.h'))
    assert set(_lib.SEARCH_SYMBOLS) == set(_header_symbols('siamese_search.h'))
    assert set(_lib.EMBED_TRAIN_SYMBOLS) == set(_header_symbols('siamese_embed_train.h'))
    assert L.sg_version() == 11000
    assert "symbols' presence" in open(os.path.join(ROOT, 'include',
                                                    'siamese_dot_embed.h')).read()


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value      # 16-byte aligned or better: ctypes arrays


def _grid_rc(L, m, mm=1, nn=1, ld_q=600, ld_db=600, ld_out=None, **null):
    """sg_dot_score_grid with dummy non-null pointers (null=0 nulls one): only paths that
    return before the first launch are exercised."""
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_dot_score_grid(m, p('q'), ld_q, p('db'), ld_db, mm, nn, 0, p('out'),
                               nn if ld_out is None else ld_out, None)


def _search_rc(L, m, mm=1, nn=4, k=1, seg=0, ld_q=600, ld_db=600, ws=None, **null):
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_dot_search_topk(m, p('q'), ld_q, p('db'), ld_db, mm, nn, 0, k, 1, seg, p('idx'),
                                p('val'), p('ws') if ws is None else ws, None)


def _train_rc(L, m, mm=1, nn=1, ld_q=600, ld_db=600, ld_lab=None, ld_s=None, batch_total=1,
              ws=None, **null):
    def p(name):
        return None if null.get(name, 1) == 0 else _P
    return L.sg_dot_score_grid_fwd_bwd(m, p('q'), ld_q, p('db'), ld_db, mm, nn, p('lab'),
                                       nn if ld_lab is None else ld_lab, batch_total, p('ys'), 1,
                                       p('s'), nn if ld_s is None else ld_s, p('gq'), p('gdb'),
                                       p('loss'), p('ws') if ws is None else ws, None)


def _refused(L, model, code=None):
    code = _lib.SG_ERR_UNSUPPORTED if code is None else code
    assert _grid_rc(L, model) == code
    assert _grid_rc(L, model, mm=0) == code                     # before the counts
    assert _search_rc(L, model) == code
    assert _train_rc(L, model) == code
    assert L.sg_dot_search_topk_workspace_bytes(model, 4, 4, 1, 0) == -1
    assert L.sg_dot_score_grid_bwd_workspace_bytes(model, 4, 4) == -1


def test_models_the_dot_calls_refuse(L):
    ntn = lib_model(problem(dict(dropout=0.0)))                  # the default NTN stack
    assert _lib.validate(ntn)[0] > 0
    _refused(L, ntn)
    web = lib_model(problem(dict(dropout=0.0), n_max=64, n_lo=5, n_hi=40), n_max=64)
    assert _lib.validate(web)[1] == _lib.PATH_WEB
    _refused(L, web)
    e513 = dot_model(27, 19)                                     # Padding of 27 rows on width 19
    assert L.sg_embed_dim(e513) == 513
    _refused(L, e513)
    _refused(L, None, _lib.SG_ERR_ARG)


def test_e512_and_small_dot_models_are_served(L):
    for rows, width in ((32, 16), (2, 3), (1, 1)):
        m = dot_model(rows, width)
        E = rows * width
        assert L.sg_embed_dim(m) == E
        assert _grid_rc(L, m, mm=0) == _lib.SG_OK
        assert _grid_rc(L, m, nn=0, q=0, db=0, out=0) == _lib.SG_OK
        assert _search_rc(L, m, mm=0, q=0, idx=0, ws=0) == _lib.SG_OK
        assert _train_rc(L, m, mm=0, q=0, gq=0, ws=0) == _lib.SG_OK
        assert _train_rc(L, m, nn=0, db=0, gdb=0, ws=0) == _lib.SG_OK
        assert L.sg_dot_search_topk_workspace_bytes(m, 4, 4, 1, 0) > 0
        assert L.sg_dot_score_grid_bwd_workspace_bytes(m, 4, 4) > 0
        # ld below E, at E
        assert _grid_rc(L, m, mm=2, nn=3, ld_q=E - 1) == _lib.SG_ERR_ARG
        assert _grid_rc(L, m, mm=2, nn=3, ld_db=E - 1) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, ld_q=E - 1) == _lib.SG_ERR_ARG
        assert _search_rc(L, m, ld_db=E - 1) == _lib.SG_ERR_ARG
        assert _train_rc(L, m, ld_q=E - 1) == _lib.SG_ERR_ARG
        assert _train_rc(L, m, ld_db=E - 1) == _lib.SG_ERR_ARG


def test_score_grid_host_validation(L):
    m = dot_model()
    assert _grid_rc(L, m, mm=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, m, nn=-1) == _lib.SG_ERR_ARG
    assert _grid_rc(L, m, mm=(1 << 29) + 1) == _lib.SG_ERR_UNSUPPORTED
    assert _grid_rc(L, m, nn=(1 << 29) + 1, q=0) == _lib.SG_ERR_UNSUPPORTED   # before pointers
    for name in ('q', 'db', 'out'):
        assert _grid_rc(L, m, mm=2, nn=3, **{name: 0}) == _lib.SG_ERR_ARG, name
    assert _grid_rc(L, m, mm=2, nn=3, ld_out=2) == _lib.SG_ERR_ARG            # ld_out < n
    # 2^23 x 2^23 tiles of 64 x 64 do not fit a launch; the pointers are fine
    assert _grid_rc(L, m, mm=1 << 29, nn=1 << 29, ld_out=1 << 29) == _lib.SG_ERR_UNSUPPORTED


def test_search_host_validation(L):
    m = dot_model()
    assert _search_rc(L, m, mm=-1) == _lib.SG_ERR_ARG
    assert _search_rc(L, m, nn=-1) == _lib.SG_ERR_ARG
    assert _search_rc(L, m, k=0) == _lib.SG_ERR_ARG
    assert _search_rc(L, m, nn=100, k=65) == _lib.SG_ERR_UNSUPPORTED
    assert _search_rc(L, m, nn=10, k=65) == _lib.SG_ERR_UNSUPPORTED           # before k > n
    assert _search_rc(L, m, nn=4, k=5) == _lib.SG_ERR_ARG                     # k > n
    assert _search_rc(L, m, nn=0, k=1) == _lib.SG_ERR_ARG                     # k > n = 0
    assert _search_rc(L, m, k=0, mm=0) == _lib.SG_ERR_ARG                     # k before m == 0
    assert _search_rc(L, m, seg=-64) == _lib.SG_ERR_ARG
    assert _search_rc(L, m, seg=100) == _lib.SG_ERR_ARG
    assert _search_rc(L, m, mm=(1 << 29) + 1, q=0) == _lib.SG_ERR_UNSUPPORTED
    for name in ('q', 'db', 'idx', 'ws'):
        assert _search_rc(L, m, **{name: 0}) == _lib.SG_ERR_ARG, name
    assert _search_rc(L, m, ws=_P + 4) == _lib.SG_ERR_ARG                     # 8-byte alignment
    for bad in ((4, 4, 0, 0), (4, 4, 65, 0), (4, 4, 5, 0), (4, 4, 1, 100), (-1, 4, 1, 0)):
        assert L.sg_dot_search_topk_workspace_bytes(m, *bad) == -1, bad
    # candidates of S segments: 12 bytes per entry; the library's own choice is sized for
    # segments of 1024 columns on every device
    assert L.sg_dot_search_topk_workspace_bytes(m, 5, 1000, 10, 64) == 16 * 5 * 10 * 12 + 256
    assert L.sg_dot_search_topk_workspace_bytes(m, 5, 1000, 10, 0) == 1 * 5 * 10 * 12 + 256
    assert L.sg_dot_search_topk_workspace_bytes(m, 5, 5000, 10, 0) == 5 * 5 * 10 * 12 + 256
    # monotone in m, n and k
    w = L.sg_dot_search_topk_workspace_bytes
    assert w(m, 6, 5000, 10, 0) > w(m, 5, 5000, 10, 0) < w(m, 5, 5000, 11, 0)
    assert w(m, 5, 6000, 10, 0) > w(m, 5, 5000, 10, 0)


def test_train_host_validation(L):
    m = dot_model()
    assert _train_rc(L, m, mm=-1) == _lib.SG_ERR_ARG
    assert _train_rc(L, m, nn=-1) == _lib.SG_ERR_ARG
    assert _train_rc(L, m, mm=(1 << 29) + 1, q=0) == _lib.SG_ERR_UNSUPPORTED
    assert _train_rc(L, m, mm=2, nn=3, ld_lab=2) == _lib.SG_ERR_ARG           # ld_labels < n
    assert _train_rc(L, m, mm=2, nn=3, ld_s=2) == _lib.SG_ERR_ARG             # ld_s < n
    assert _train_rc(L, m, mm=2, nn=3, ld_s=2, s=0, ws=0) == _lib.SG_ERR_ARG  # the workspace
    for name in ('q', 'db', 'gq', 'gdb', 'ws', 'ys'):                          # broadcast: y_stats
        assert _train_rc(L, m, mm=2, nn=3, **{name: 0}) == _lib.SG_ERR_ARG, name
    assert _train_rc(L, m, mm=2, nn=3, ws=_P + 8) == _lib.SG_ERR_ARG          # 16-byte alignment
    al = dot_model(loss_mode='aligned')
    assert _train_rc(L, al, mm=2, nn=3, lab=0) == _lib.SG_ERR_ARG
    assert _train_rc(L, al, mm=2, nn=3, batch_total=0) == _lib.SG_ERR_ARG
    w = L.sg_dot_score_grid_bwd_workspace_bytes
    assert w(m, -1, 5) == -1 and w(None, 3, 5) == -1 and w(m, 3, (1 << 29) + 1) == -1
    assert w(m, 1 << 29, 1 << 29) == -1                                        # GS [m][n]
    # the header's formula, E = 6: GS, tile partials, partial products per 512 rows
    up = lambda x: (x + 63) & ~63
    for mm, nn in ((1, 1), (5, 65), (700, 700), (513, 1025), (0, 7)):
        want = up(mm * nn) + up(-(-mm // 64) * -(-nn // 64)) + up(-(-nn // 512) * mm * 6) + \
            up(-(-mm // 512) * nn * 6)
        assert w(m, mm, nn) == want * 4 + 256, (mm, nn)
    assert w(m, 700, 701) >= w(m, 700, 700) <= w(m, 701, 700)


def test_only_the_training_call_refuses_dropout(L):
    dropped = dot_model(keep_prob=0.9)
    assert _train_rc(L, dropped) == _lib.SG_ERR_UNSUPPORTED
    assert _train_rc(L, dropped, mm=0) == _lib.SG_ERR_UNSUPPORTED              # before the counts
    assert L.sg_dot_score_grid_bwd_workspace_bytes(dropped, 4, 4) == -1
    # the inference calls read keep_prob as 1
    assert _grid_rc(L, dropped, mm=0) == _lib.SG_OK
    assert _grid_rc(L, dropped, mm=2, nn=3, out=0) == _lib.SG_ERR_ARG          # accepted: next check
    assert _search_rc(L, dropped, idx=0) == _lib.SG_ERR_ARG
    assert L.sg_dot_search_topk_workspace_bytes(dropped, 4, 4, 1, 0) > 0
    # keep_prob = 1 is the copy Python passes under dropout='graph'
    assert _train_rc(L, dot_model(keep_prob=1.0), mm=0) == _lib.SG_OK
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        _lib.dot_score_grid_bwd_workspace_bytes(dropped, 4, 4)


def test_old_calls_still_refuse_the_dot_head(L):
    dot = dot_model()
    assert _lib.validate(dot)[0] > 0
    assert L.sg_score_grid_workspace_bytes(dot, 4) == -1
    assert L.sg_score_grid(dot, _P, _P, 1, 1, _P, 0, _P, 1, _P, None) == _lib.SG_ERR_UNSUPPORTED
    assert L.sg_search_topk_workspace_bytes(dot, 4, 4, 1, 0) == -1
    assert L.sg_search_topk(dot, _P, _P, 1, 4, _P, 0, 1, 1, 0, _P, _P, _P, None) == \
        _lib.SG_ERR_UNSUPPORTED
    assert L.sg_score_grid_bwd_workspace_bytes(dot, 4, 4) == -1
    assert L.sg_score_grid_fwd_bwd(dot, _P, _P, 1, 1, _P, _P, 1, 1, _P, 1, _P, 1, _P, _P, _P, _P,
                                   _P, None) == _lib.SG_ERR_UNSUPPORTED
    with pytest.raises(_lib.SiameseHipError):
        _lib.score_grid_workspace_bytes(dot, 4)
    # the node-stack calls serve it, as before
    assert L.sg_embed_dim(dot) == 6
    assert L.sg_embed_bwd_workspace_bytes(dot, 4) > 0
