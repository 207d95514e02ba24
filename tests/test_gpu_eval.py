"""Device-side evaluation of the test matrix on the GPU (include/siamese_eval.h).

sg_eval_rows' integer outputs are compared exactly with what results.py's top_k_ids and
ranking give per row (a SiameseModelResult of the float32 scores cast to float64 against a
DistanceMatrixResult given both distance matrices), on shapes around the 64-lane and
256-column steps of the kernel, with heavy ties, and at the largest row it serves; sqerr
against the float64 numpy row sums at rtol 1e-9 (a sum of N <= 1e5 non-negative float64
terms differs between any two orders by at most N * 2^-52 = 2.2e-11 relative; the bound is
wider only to be independent of the reduction shape); then train.test(eval_path='device')
against eval_path='host' on the same model, fused and graph-store."""
import numpy as np
import pytest

from _embed_fixtures import ntn_stack

pytestmark = pytest.mark.gpu

EVAL_KS = (1, 2, 5, 10, 20, 50, 100)
SQ_RTOL = 1e-9


def _eval_ks(n):
    return tuple(k for k in EVAL_KS if k < n)


# name: (m, n, ld or None, ks)
SHAPES = {
    '1x2': (1, 2, None, (1,)),
    '3x63': (3, 63, None, _eval_ks(63)),
    '3x64': (3, 64, None, _eval_ks(64)),
    '5x65': (5, 65, None, _eval_ks(65)),
    '37x70_ld96': (37, 70, 96, (1, 2, 5, 10, 20, 50)),
    '4x130': (4, 130, None, _eval_ks(130)),
    '4x130_kmax': (4, 130, None, _eval_ks(130) + (129,)),
    '2x1000': (2, 1000, None, _eval_ks(1000)),
    '1x32768': (1, 32768, None, (1, 10, 100)),
}
QUANT = np.array([-1.0, -0.0, 0.0, 0.5, 2.0], dtype=np.float32)   # both zeros: they tie
VARIANTS = ('plain', 'ties', 'eq_scores', 'eq_dist')


def _problem(name, variant):
    """scores float32 [m][n], the two true distance matrices and true similarities."""
    m, n, _, _ = SHAPES[name]
    rng = np.random.default_rng(sorted(SHAPES).index(name) * 7 + VARIANTS.index(variant))
    if variant == 'plain':
        scores = rng.standard_normal((m, n)).astype(np.float32)
        if n > 1000:   # distinct true distances: the candidates stay near kmax
            d = np.stack([rng.permutation(n) for _ in range(m)]).astype(np.float64)
        else:          # GED-like: small integers, some ties
            d = rng.integers(0, max(4, n // 3), size=(m, n)).astype(np.float64)
    else:   # every graph a candidate; scores of five values
        scores = QUANT[rng.integers(0, len(QUANT), size=(m, n))]
        d = rng.integers(0, 4, size=(m, n)).astype(np.float64)
        if n >= 63:
            zeros = np.signbit(scores[scores == 0])
            assert zeros.any() and not zeros.all()
        for q in {0, m - 1}:
            if variant == 'eq_scores':
                scores[q] = 0.5
            if variant == 'eq_dist':
                d[q] = 2.0
    dn = d / (1.0 + rng.integers(0, 3, size=(m, n)))     # another tie pattern for norm=True
    sim = np.exp(-0.6 * dn * dn)
    return scores, d, dn, sim


def _host_counts(scores, d, dn, norm, ks):
    """hits [m][nk] and best [m] per row with Result.top_k_ids and Result.ranking."""
    from graphembedding_amd.results import DistanceMatrixResult, SiameseModelResult
    m, n = scores.shape
    true = DistanceMatrixResult('none', 'astar', d, dn)          # _normalize is never called
    pred = SiameseModelResult('none', 'siamese_test', sim_mat=scores.astype(np.float64),
                              time_mat=np.zeros((m, n)))
    order = pred.sort_id_mat_                  # sort_id_mat() of the constructor: the same
    pred.sort_id_mat = lambda norm=False: order   # sort, once instead of once per call
    hits = np.zeros((m, len(ks)), dtype=np.int64)
    best = np.zeros(m, dtype=np.int64)
    for q in range(m):
        for c, k in enumerate(ks):
            truth = set(true.top_k_ids(q, k, norm, inclusive=True))
            guess = set(pred.top_k_ids(q, k, norm, inclusive=False))
            hits[q][c] = len(truth & guess)
        tops = np.asarray(true.top_k_ids(q, 1, norm, inclusive=True))
        if len(tops) > 64:
            # ranking resolves ties to the best rank, so it depends on the score alone: one
            # true top-1 graph per distinct score gives the same minimum
            _, first = np.unique(scores[q][tops], return_index=True)
            tops = tops[first]
        best[q] = min(pred.ranking(q, int(t), norm, one_based=True) for t in tops)
    return hits, best


def _device_counts(gpu, scores, ld, dist, sim, ks):
    import torch
    from graphembedding_amd.device_eval import eval_counts, true_ranks
    m, n = scores.shape
    buf = torch.full((m, ld or n), -7.25, dtype=torch.float32, device=gpu)
    buf[:, :n] = torch.from_numpy(scores).to(gpu)
    view = buf[:, :n]
    tr = torch.from_numpy(true_ranks(dist)).to(gpu)
    ts = None if sim is None else torch.from_numpy(np.ascontiguousarray(sim)).to(gpu)
    hits, best, sqerr, nans = eval_counts(view, tr, ts, ks)
    return (hits.cpu().numpy(), best.cpu().numpy(),
            None if sqerr is None else sqerr.cpu().numpy(), nans.cpu().numpy())


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('name', list(SHAPES))
def test_eval_rows_integer_parity(gpu, name, variant):
    m, n, ld, ks = SHAPES[name]
    scores, d, dn, sim = _problem(name, variant)
    for norm, dist in ((False, d), (True, dn)):
        want_hits, want_best = _host_counts(scores, d, dn, norm, ks)
        hits, best, sqerr, nans = _device_counts(gpu, scores, ld, dist, sim, ks)
        assert hits.shape == (m, len(ks)) and hits.dtype == np.int32
        assert np.array_equal(hits, want_hits), (name, variant, norm)
        assert np.array_equal(best, want_best), (name, variant, norm)
        assert not nans.any()
        want_sq = ((sim - scores.astype(np.float64)) ** 2).sum(axis=1)
        np.testing.assert_allclose(sqerr, want_sq, rtol=SQ_RTOL, atol=0)
    if variant == 'eq_scores':   # ties to the larger column: the last k columns are the guess
        assert want_best[0] == 1


def test_eval_rows_sqerr_is_reproducible_and_optional(gpu):
    name = '37x70_ld96'
    m, n, ld, ks = SHAPES[name]
    scores, d, dn, sim = _problem(name, 'ties')
    a = _device_counts(gpu, scores, ld, d, sim, ks)
    b = _device_counts(gpu, scores, ld, d, sim, ks)
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))   # the same bits
    c = _device_counts(gpu, scores, ld, d, None, ks)                    # true_sim = NULL
    assert c[2] is None
    for x, y in ((a[0], c[0]), (a[1], c[1]), (a[3], c[3])):
        assert np.array_equal(x, y)
    big = _problem('1x32768', 'plain')
    a = _device_counts(gpu, big[0], None, big[1], big[3], (1, 10, 100))
    b = _device_counts(gpu, big[0], None, big[1], big[3], (1, 10, 100))
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


def _truth(gpu, d, dn):
    from graphembedding_amd.device_eval import TruthTable
    from graphembedding_amd.results import DistanceMatrixResult
    true = DistanceMatrixResult('none', 'astar', d, dn)
    return true, TruthTable(true, 'gaussian', 0.6, gpu)


def test_eval_rows_counts_nans_and_python_raises(gpu):
    import torch
    from graphembedding_amd import device_eval
    name = '5x65'
    m, n, ld, ks = SHAPES[name]
    scores, d, dn, sim = _problem(name, 'plain')
    scores[2, 64] = np.nan
    nans = _device_counts(gpu, scores, ld, d, sim, ks)[3]
    assert nans.tolist() == [0, 0, 1, 0, 0]
    _, truth = _truth(gpu, d, dn)
    with pytest.raises(ValueError, match='NaN'):
        device_eval.eval_rows(torch.from_numpy(scores).to(gpu), truth, False)
    scores[2, 64] = 0.25
    device_eval.eval_rows(torch.from_numpy(scores).to(gpu), truth, False)


@pytest.mark.parametrize('variant', ('plain', 'ties'))
def test_device_eval_matches_metrics(gpu, variant):
    """device_eval.eval_rows against metrics.py on the same matrix: the aps and the MRR bit
    for bit, the mse within SQ_RTOL."""
    import torch
    from graphembedding_amd import device_eval, metrics
    from graphembedding_amd.results import SiameseModelResult
    scores, d, dn, _ = _problem('37x70_ld96', variant)
    m, n = scores.shape
    true, truth = _truth(gpu, d, dn)
    assert truth.ks == [1, 2, 5, 10, 20, 50]
    pred = SiameseModelResult('none', 'siamese_test', sim_mat=scores.astype(np.float64),
                              time_mat=np.zeros((m, n)))
    dev = torch.from_numpy(scores).to(gpu)
    for norm in (True, False):
        aps, mrr, mse = device_eval.eval_rows(dev, truth, norm)
        assert np.array_equal(aps, metrics.precision_at_ks(true, pred, norm, truth.ks))
        assert mrr == metrics.mean_reciprocal_rank(true, pred, norm)
        np.testing.assert_allclose(mse, metrics.mean_squared_error(true, pred, 'gaussian', 0.6,
                                                                   norm), rtol=SQ_RTOL, atol=0)


# ---- end to end ---------------------------------------------------------------------------
_RUNS = {}


def _trained(gpu, kind):
    """main() on the AIDS80nef-shaped data (10 x 70), once per kind of model."""
    if kind not in _RUNS:
        from graphembedding_amd.config import Flags
        from graphembedding_amd.train import main
        if kind == 'web':   # the fixture of test_gpu_web_embed.test_train_test_embed_path_web
            f = Flags(dataset='syn_aids80nef', iters=2, n_max=64, node_feat_order='sorted',
                      dropout=0.0, **ntn_stack(64, 10))
        else:
            f = Flags(dataset='syn_aids80nef', iters=2, n_max=10, node_feat_order='sorted')
        _, _, (data, dc, model) = main(f, device=gpu, return_objects=True)
        assert model.is_web == (kind == 'web')
        _RUNS[kind] = (f, data, dc, model)
    return _RUNS[kind]


@pytest.mark.parametrize('kind', ('fused', 'web'))
def test_train_test_device_eval_matches_host(gpu, kind):
    from graphembedding_amd.eval import Eval
    from graphembedding_amd.train import test
    f, data, dc, model = _trained(gpu, kind)
    out = {}
    for path in ('host', 'device'):
        ev = Eval.from_calculator(data, dc, f)
        sim_mat, time_mat, res = test(data, dc, model, f.copy(test_path='embed', eval_path=path),
                                      ev, verbose=False)
        assert sim_mat.shape == time_mat.shape == (10, 70)
        out[path] = (sim_mat, res)
    assert np.array_equal(out['host'][0], out['device'][0])     # inference mode: the same matrix
    host, dev = out['host'][1], out['device'][1]
    assert set(host) == set(dev) and 'time' in dev and 'time_mat_mode' in dev
    name = f.model
    for key in host:
        assert set(host[key]) == set(dev[key]) == {name}, key
    assert dev['time_mat_mode'] == host['time_mat_mode']
    assert dev['time'][name] > 0
    for sfx in ('_norm', '_nonorm'):
        assert dev['apk' + sfx][name]['ks'] == host['apk' + sfx][name]['ks'] == \
            [1, 2, 5, 10, 20, 50]
        assert set(dev['apk' + sfx][name]) == set(host['apk' + sfx][name])
        assert np.array_equal(dev['apk' + sfx][name]['aps'], host['apk' + sfx][name]['aps'])
        assert dev['mrr' + sfx][name] == host['mrr' + sfx][name]
        np.testing.assert_allclose(dev['mse' + sfx][name], host['mse' + sfx][name],
                                   rtol=SQ_RTOL, atol=0)
        print(kind, sfx, 'aps', dev['apk' + sfx][name]['aps'], 'mrr', dev['mrr' + sfx][name],
              'mse', dev['mse' + sfx][name], host['mse' + sfx][name])


def test_device_eval_refusals(gpu):
    from graphembedding_amd.eval import Eval
    from graphembedding_amd.train import test
    f, data, dc, model = _trained(gpu, 'fused')
    ev = Eval.from_calculator(data, dc, f)
    for bad in (dict(test_path='pairs'), dict(test_path='embed', test_matrix='compat_diag'),
                dict(test_path='pairs', test_matrix='compat_diag')):
        with pytest.raises(RuntimeError, match="eval_path='device'"):
            test(data, dc, model, f.copy(eval_path='device', **bad), ev, verbose=False)
    with pytest.raises(RuntimeError, match='Unknown eval_path'):
        test(data, dc, model, f.copy(test_path='embed', eval_path='gpu'), ev, verbose=False)
    assert not ev.results
