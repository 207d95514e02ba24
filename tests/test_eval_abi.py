"""Host side of the device evaluation (include/siamese_eval.h): the library exports exactly
the header's symbols next to the unchanged other headers' sets, sg_eval_rows checks every
argument rule of the header before any HIP call (dummy pointers, so all of this runs without
a GPU), the eval_path flag defaults to the host, and device_eval.true_ranks reproduces the
tie-inclusive true top-k sets of results.py."""
import ctypes
import os
import re

import numpy as np
import pytest

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
                 'siamese_web_embed_train.h': 'WEB_EMBED_TRAIN_SYMBOLS',
                 'siamese_web_embed_drop.h': 'WEB_EMBED_DROP_SYMBOLS'}
A, U, OK = _lib.SG_ERR_ARG, _lib.SG_ERR_UNSUPPORTED, _lib.SG_OK


@pytest.fixture(scope='module')
def L():
    build_hip()
    return _lib.lib()


def _header_symbols(name):
    src = open(os.path.join(ROOT, 'include', name)).read()
    return sorted(set(re.findall(SYM_RE, src, re.M)))


def test_eval_header_symbols_are_exported(L):
    syms = _header_symbols('siamese_eval.h')
    assert set(syms) == set(_lib.EVAL_SYMBOLS), syms
    assert len(_lib.EVAL_SYMBOLS) == len(set(_lib.EVAL_SYMBOLS)) == 2
    for s in syms:
        assert hasattr(L, s), s
    for fn in ('eval_workspace_bytes', 'eval_rows'):
        assert callable(getattr(_lib, fn)), fn
    assert L.sg_version() == 11000


def test_eval_symbols_are_disjoint_from_the_other_headers():
    for header, name in OTHER_HEADERS.items():
        other = getattr(_lib, name)
        assert not set(_lib.EVAL_SYMBOLS) & set(other), name
        assert set(other) == set(_header_symbols(header)), header     # the others are unchanged


_BUF = (ctypes.c_float * 64)()
_P = ctypes.cast(_BUF, ctypes.c_void_p).value


def _rc(L, m=3, n=70, ld=None, ks=(1, 2, 5, 10, 20, 50), nk=None, sim=1, sq=1, **null):
    """sg_eval_rows with dummy non-null pointers (name=0 passes NULL): only paths that return
    before the launch are exercised.  ks=None passes a NULL array of nk entries."""
    p = lambda name: None if null.get(name) == 0 else _P   # noqa: E731
    arr = None if ks is None else (ctypes.c_int32 * max(len(ks), 1))(*ks)
    nk = len(ks) if nk is None else nk
    return L.sg_eval_rows(p('scores'), m, n, n if ld is None else ld, p('tr'),
                          _P if sim else None, arr, nk, p('hits'), p('best'),
                          _P if sq else None, p('nan'), None, None)


def test_eval_argument_rules(L):
    """The header's table, rule by rule; the workspace query refuses the same m, n and nk."""
    ws = L.sg_eval_rows_workspace_bytes
    # nk < 1, ks not strictly ascending, ks[0] < 1, ks[nk-1] >= n
    assert _rc(L, ks=()) == A and ws(3, 70, 0) == -1
    assert _rc(L, nk=-1) == A and ws(3, 70, -1) == -1
    assert _rc(L, ks=None, nk=2) == A
    assert _rc(L, ks=(1, 5, 5)) == A
    assert _rc(L, ks=(1, 10, 5)) == A
    assert _rc(L, ks=(0, 1, 2)) == A
    assert _rc(L, ks=(-3, 1)) == A
    assert _rc(L, ks=(1, 2, 70)) == A
    assert _rc(L, m=0, ks=(1, 2, 70)) == A
    assert _rc(L, m=0, ks=(1, 2, 69)) == OK              # n - 1 is the largest k
    assert _rc(L, n=2, ks=(1, 2)) == A
    assert _rc(L, m=0, n=2, ks=(1,)) == OK
    assert _rc(L, n=1, ks=(1,)) == A and ws(3, 1, 1) == -1
    assert _rc(L, n=0, ks=(1,)) == A and ws(3, 0, 1) == -1
    assert ws(3, 5, 5) == -1 and ws(3, 5, 4) == 0        # no 5 ascending k's within [1, 5)
    # nk > 16
    assert _rc(L, n=100, ks=tuple(range(1, 18))) == U and ws(3, 100, 17) == -1
    assert _rc(L, n=10, ks=tuple(range(1, 18))) == U     # before ks is looked at
    assert _rc(L, n=100, ks=tuple(range(1, 17)), scores=0) == A   # 16 k's are served
    assert ws(3, 100, 16) == 0
    # negative sizes, ld < n
    assert _rc(L, m=-1) == A and ws(-1, 70, 6) == -1
    assert _rc(L, n=-1) == A and ws(3, -1, 6) == -1
    assert _rc(L, ld=-1) == A
    assert _rc(L, ld=69) == A
    assert _rc(L, ld=96, scores=0) == A                  # ld > n is fine: on to the pointers
    # exactly one of true_sim and sqerr_out
    assert _rc(L, sim=0) == A
    assert _rc(L, sq=0) == A
    assert _rc(L, sim=0, sq=0, scores=0) == A            # both NULL is fine
    # n > 32768, m > 2^29
    assert _rc(L, n=32769) == U and ws(3, 32769, 6) == -1
    assert _rc(L, n=32768, scores=0) == A and ws(3, 32768, 6) == 0
    assert _rc(L, m=(1 << 29) + 1) == U and ws((1 << 29) + 1, 70, 6) == -1
    assert _rc(L, m=1 << 29, scores=0) == A and ws(1 << 29, 70, 6) == 0
    # m == 0: no work, whatever the pointers; the argument checks still come first
    assert _rc(L, m=0, scores=0, tr=0, hits=0, best=0, nan=0) == OK
    assert ws(0, 70, 6) == 0
    assert _rc(L, m=0, ks=(5, 1)) == A
    assert _rc(L, m=0, ld=3) == A
    assert _rc(L, m=0, sim=0) == A
    assert _rc(L, m=0, n=32769) == U
    assert _rc(L, m=0, n=100, ks=tuple(range(1, 18))) == U
    # the pointers, still on the host
    for null in ('scores', 'tr', 'hits', 'best', 'nan'):
        assert _rc(L, **{null: 0}) == A, null
    with pytest.raises(_lib.SiameseHipError, match='sg_eval_rows_workspace_bytes'):
        _lib.eval_workspace_bytes(3, 32769, 6)
    assert _lib.eval_workspace_bytes(3, 70, 6) == 0


def test_eval_path_flag_defaults_to_host():
    from graphembedding_amd.config import DEFAULTS, Flags
    assert Flags().eval_path == 'host' == DEFAULTS['eval_path']


@pytest.mark.parametrize('seed,m,n,hi', [(0, 4, 9, 3), (1, 6, 40, 4), (2, 3, 130, 7),
                                         (3, 2, 64, 1), (4, 5, 33, 1000)])
def test_true_ranks_match_tie_inclusive_top_k(seed, m, n, hi):
    """{j : tr[q][j] < k} is top_k_ids(q, k, norm, inclusive=True), for every q, every k the
    host accepts and both norms, on integer-valued distances with heavy ties (hi = 1: one
    value, every graph tied)."""
    from graphembedding_amd.device_eval import true_ranks
    from graphembedding_amd.results import DistanceMatrixResult
    rng = np.random.default_rng(seed)
    d = rng.integers(0, hi, size=(m, n)).astype(np.float64)
    dn = rng.integers(0, hi, size=(m, n)).astype(np.float64) / 4.0
    true = DistanceMatrixResult('none', 'astar', d, dn)
    for norm, mat in ((True, dn), (False, d)):
        tr = true_ranks(mat)
        assert tr.dtype == np.int32 and tr.shape == (m, n)
        assert np.array_equal(tr, (mat[:, None, :] < mat[:, :, None]).sum(axis=2))
        for q in range(m):
            for k in range(1, n):
                want = set(int(j) for j in true.top_k_ids(q, k, norm, inclusive=True))
                assert set(np.flatnonzero(tr[q] < k).tolist()) == want, (q, k, norm)
            assert set(np.flatnonzero(tr[q] == 0).tolist()) == \
                set(int(j) for j in true.top_k_ids(q, 1, norm, inclusive=True))
