"""The float64 reference of the NTN head that test_gpu_web_grid_shapes.py measures
sg_web_score_grid against (_embed_fixtures.ntn_head_ref), checked on the CPU:
(1) on real embeddings from the oracle's node stack it agrees with the oracle's pair forward;
(2) with the synthetic signed embeddings and the parameters of every model the GPU file uses,
    dropping any one of four terms of the head moves nearly every score by far more than the
    GPU tolerance, so a kernel that got that term wrong could not pass."""
import numpy as np
import pytest

from _embed_fixtures import (GRID_REF_MODELS, grid_ref_embeddings, grid_ref_problem,
                             ntn_head_params, ntn_head_ref, oracle_graphs)
from oracle import siamese_oracle as O
from test_gpu_web_embed import _grid_problem, _oracle_embeddings

TOL = 1e-4          # the GPU file's per-pair bar
MOVE = 10 * TOL     # a removed term must move a score by more than this ...
SHARE = 0.9         # ... for at least this share of the scores


@pytest.mark.parametrize('kw', [dict(), dict(ntn_mode='intended'), dict(bias=False)],
                         ids=['reference', 'intended', 'no_bias'])
def test_head_ref_matches_oracle_forward(kw):
    """D = 64, K = 10, a 5 x 37 grid of the oracle's own embeddings: ntn_head_ref agrees with
    O.forward (node stack and head) to 1e-9."""
    m, n = 5, 37
    prob = _grid_problem(64, **kw)
    emb = _oracle_embeddings(prob)
    G = emb.shape[0]
    assert (emb != 0).mean() > 0.2                       # not the all-zero embedding
    rng = np.random.default_rng(7)
    qi, di = rng.integers(0, G, size=m), rng.integers(0, G, size=n)
    W, V, bias, U = ntn_head_params(prob)
    assert (bias is None) == (kw.get('bias') is False)
    got = ntn_head_ref(emb[qi], emb[di], W, V, bias, U, prob.flags.ntn_mode, 10)
    gs = oracle_graphs(prob)
    want = O.forward(prob.oracle_spec(), prob.params.astype(np.float64),
                     [gs[i] for i in np.repeat(qi, n)], [gs[j] for j in np.tile(di, m)],
                     0).reshape(m, n)
    print('max |ref - oracle|', float(np.abs(got - want).max()), 'max |score|',
          float(np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)
    assert np.ptp(want) > 100 * TOL                       # the scores differ between pairs


def test_head_ref_final_act():
    prob = grid_ref_problem(32, 10)
    W, V, bias, U = ntn_head_params(prob)
    eq, edb = grid_ref_embeddings(32, 2, 3)
    pre = ntn_head_ref(eq, edb, W, V, bias, U, 'reference', 10)
    act = ntn_head_ref(eq, edb, W, V, bias, U, 'reference', 10, final_act=lambda x: 2.0 * x + 1)
    assert np.array_equal(act, 2.0 * pre + 1)


def _without(W, V, bias, what):
    """The head's parameters with one term removed."""
    D = W.shape[0]
    W, V = W.copy(), V.copy()
    if what == 'a=D-1':            # the last index of the contraction with e_i
        W[D - 1, :, :] = 0.0
    elif what == 'b=D-1':          # the last index of the contraction with e_j
        W[:, D - 1, :] = 0.0
    elif what == 'bias_row':       # V[k][:D] · e_i + bias[k]: what multiplies the 1 of [e_j, 1]
        V[:, :D] = 0.0
        bias = None
    elif what == 'V_ej':           # V[k][D:] · e_j
        V[:, D:] = 0.0
    else:
        raise ValueError(what)
    return W, V, bias


@pytest.mark.parametrize('D,K,bias,ntn_mode', GRID_REF_MODELS)
def test_removed_terms_move_the_scores(D, K, bias, ntn_mode):
    """The condition that makes a pass of the GPU comparison meaningful, for the parameters
    and embeddings (first rows) of every GPU case."""
    prob = grid_ref_problem(D, K, bias, ntn_mode)
    W, V, b, U = ntn_head_params(prob)
    assert (b is None) == (not bias)
    eq, edb = grid_ref_embeddings(D, 5, 37)
    assert eq.dtype == np.float32 and (eq < 0).any() and (eq > 0).any() and (eq != 0).all()
    full = ntn_head_ref(eq, edb, W, V, b, U, ntn_mode, K)
    for what in ('a=D-1', 'b=D-1', 'bias_row', 'V_ej'):
        Wx, Vx, bx = _without(W, V, b, what)
        moved = np.abs(ntn_head_ref(eq, edb, Wx, Vx, bx, U, ntn_mode, K) - full)
        share = float((moved > MOVE).mean())
        print('D', D, 'K', K, what, 'share moved', share, 'median move', float(np.median(moved)))
        assert share >= SHARE, (D, K, what, share)
