"""bench.py as a command: a plain run's result line and the arrays --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                        '--steps', '3', '--warmup', '1', '--settle-ms', '0',
                        '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['full'] is False
    assert line['unit'] == 'graph-pairs/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'f32'
    # value and ms_per_step are the same measurement
    assert line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(
        line['config']['global_batch'] / (line['ms_per_step'] * 1e-3), rel=1e-9)
    # what only --full measures is null in a plain line
    for k in ('roofline', 'roofline_hbm', 'cpu_baseline', 'forward_pairs_per_s'):
        assert line[k] is None, k
    assert line['config']['pack_ms'] is None and line['config']['order_ms'] is None
    assert line['event_steps_after_timed'] == 0

    assert sorted(os.listdir(out)) == ['adam_m.npy', 'adam_v.npy', 'grad.npy', 'loss.npy',
                                       'params.npy']
    a = {n: np.load(out / (n + '.npy')) for n in ('params', 'grad', 'adam_m', 'adam_v', 'loss')}
    for n, x in a.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
    assert a['params'].ndim == 1 and a['params'].size > 0
    assert a['grad'].shape == a['adam_m'].shape == a['adam_v'].shape == a['params'].shape
    assert np.any(a['grad'] != 0) and np.all(a['adam_v'] >= 0)
    # [loss_mse, regularisation] of the last timed step: the line's loss is their sum
    assert a['loss'].shape == (2,)
    assert float(a['loss'][0]) + float(a['loss'][1]) == line['loss']
