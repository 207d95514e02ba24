"""Host Eval.eval_test against the device Eval.eval_test_device (GPU only).

    python scripts/eval_bench.py [--repeats 5] [--out FILE.json]

Both turn the same m x n score matrix into ap@k, MRR and "mse" for both norms; the scores are
synthetic (uniform float32), the true distances GED-like small integers (Poisson, mean 8), so
the true top-k sets carry ties as on the labelled sets.  Shapes: AIDS700nef (140 x 560) and C4 (AIDS10knef, 2,000 x 8,000).
Each side is timed with its own synchronised wall clock after a warm-up call:
  host    one Eval.eval_test (metrics.py over results.py's sorts) of the float64 matrix.
          For C4 it is timed on the FIRST 8 QUERY ROWS ONLY and scaled by 2000 / 8: a lower
          bound, because every sort of the full pass would cover all 2,000 rows;
  device  the median of --repeats Eval.eval_test_device calls on the float32 device matrix
          (two sg_eval_rows launches and the copies of the per-row counts), with the
          TruthTable already built; its one-off build and upload is reported next to it.
Before timing, the device aps and MRR must equal the host's bit for bit and the mse within
1e-9 (for C4 on the 8 rows the host evaluates).  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL = 'siamese_gcntn_mse'
SHAPES = (('aids700nef', 140, 560, None), ('c4_aids10knef', 2000, 8000, 8))


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


def _problem(m, n, seed):
    rng = np.random.default_rng(seed)
    d = rng.poisson(8.0, size=(m, n)).astype(np.float64)   # GED-like: few graphs tie at the top
    dn = d / (0.5 * rng.integers(10, 21, size=(m, 1)) + 0.5 * rng.integers(10, 21, size=(1, n)))
    scores = rng.random((m, n), dtype=np.float32)
    return scores, d, dn


def _evaluator(d, dn):
    from graphembedding_amd.eval import Eval
    from graphembedding_amd.results import DistanceMatrixResult
    true = DistanceMatrixResult('bench', 'astar', d, dn)
    return Eval('bench', 'astar', 'gaussian', 0.6, true_result=true)


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000.0, out


def _same(host, dev):
    for sfx in ('_norm', '_nonorm'):
        assert np.array_equal(host['apk' + sfx][MODEL]['aps'], dev['apk' + sfx][MODEL]['aps'])
        assert host['mrr' + sfx][MODEL] == dev['mrr' + sfx][MODEL]
        np.testing.assert_allclose(dev['mse' + sfx][MODEL], host['mse' + sfx][MODEL],
                                   rtol=1e-9, atol=0)


def bench_shape(name, m, n, host_rows, repeats, device):
    import torch
    scores, d, dn = _problem(m, n, m + n)
    time_mat = np.ones((m, n))
    dev_scores = torch.from_numpy(scores).to(device)
    ev = _evaluator(d, dn)
    build_ms, res = _wall(lambda: dict(ev.eval_test_device(MODEL, dev_scores, time_mat)))
    dev_ms = sorted(_wall(lambda: ev.eval_test_device(MODEL, dev_scores, time_mat))[0]
                    for _ in range(repeats))
    r = host_rows or m
    hev = _evaluator(d[:r], dn[:r])
    sims = scores[:r].astype(np.float64)
    warm = min(r, 4)
    _evaluator(d[:warm], dn[:warm]).eval_test(MODEL, sims[:warm], time_mat[:warm])   # warm-up
    host_ms, host = _wall(lambda: dict(hev.eval_test(MODEL, sims, time_mat[:r])))
    if host_rows:   # the device result of the same rows
        dev_part = dict(_evaluator(d[:r], dn[:r]).eval_test_device(
            MODEL, dev_scores[:r].contiguous(), time_mat[:r]))
        _same(host, dev_part)
    else:
        _same(host, res)
    out = dict(shape=name, m=m, n=n, ks=res['apk_norm'][MODEL]['ks'],
               device_ms_median=dev_ms[len(dev_ms) // 2], device_ms_min=dev_ms[0],
               device_ms_max=dev_ms[-1], device_repeats=repeats,
               device_first_call_ms_with_truth_table=build_ms,
               host_rows_timed=r, host_ms_timed=host_ms)
    if host_rows:
        out['host_ms_scaled'] = host_ms * m / r
        out['host_note'] = ('host timed on the first {} query rows only and scaled by {} / {}: '
                            'a lower bound, the full pass sorts all {} rows per call'
                            .format(r, m, r, m))
    else:
        out['host_ms_scaled'] = host_ms
    out['host_over_device'] = out['host_ms_scaled'] / out['device_ms_median']
    return out


def main():
    import torch
    from graphembedding_amd.build import build_hip
    build_hip()
    device = torch.device('cuda:0')
    repeats = _arg('--repeats', 5)
    result = dict(bench='eval_device', gpu=torch.cuda.get_device_name(0),
                  shapes=[bench_shape(name, m, n, rows, repeats, device)
                          for name, m, n, rows in SHAPES])
    line = json.dumps(result)
    print(line)
    out = _arg('--out', '')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
