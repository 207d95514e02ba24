"""Cases and witnesses of tests/test_gpu_schedule.py, and the child process it starts.

    python tests/_schedule_child.py CASE [CASE ...]

runs the named cases under the environment it was started with (SG_CLS_W, SG_XCD_W,
SG_FAST_WAVES: the library reads them once per process) and prints one JSON line.  The
test module imports this file too: its in-process cases go through the same `run_case`,
and every result, the child's or its own, through the same `check_result`.

The child does not judge results.  It asserts only that a case reaches the branch of the
pair schedule it was built for (`restate`), and leaves the rest to `check_result`."""
import time

T_START = time.time()

import json  # noqa: E402
import os  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402

from _fixtures import check_grad_per_var, run_oracle_step, small_problem  # noqa: E402

# a reassociated fp32 sum over at most 4096 pairs (test_gpu_parity.test_large_batch_properties)
TOL = 1e-5
MAX_PAIRS = 4096
# against the oracle (test_gpu_parity.TOL), for cases the oracle can run
ORACLE_TOL = 1e-4
ORACLE_PAIRS = 40
SEED = 4242
# Every label is LABEL, outside the range (0, 1] of the predictions exp(-yeta s^2): with
# ybar = LABEL each pair adds ((yhat - LABEL)^2) / 2, between 1/2 and 2, to the loss, so no
# pair's share of the loss is below 1 / (4 n_pairs) >= 6.1e-5 * (4096 / n_pairs); natural
# labels leave pairs with yhat ~ ybar, whose loss the sensitivity guard could not see.
LABEL = 2.0

# ---- the wave split, restated (selects inputs only; never a reference for results) ----
CW_BWD = (1.0, 1.355, 1.351, 1.546)   # default stack, f32 records, forward + backward
CW_FWD = (1.0, 1.28, 1.28, 1.44)      # forward only
Q_MANY = 64                           # a class's waves hold "many pairs" from here on


def class_weights(bwd):
    ev = os.environ.get('SG_CLS_W')
    if ev:
        w = [float(x) for x in ev.split(',')]
        assert len(w) == 4 and all(x > 0 for x in w), ev
        return tuple(w)
    return CW_BWD if bwd else CW_FWD


def waves_per_block():
    return int(os.environ.get('SG_FAST_WAVES', '0')) or 8


def unit_counts(counts, cw, units):
    """Units (SIMD pairs at 8 waves per block, else waves) per class: in proportion to
    count x weight by largest remainder, one unit per non-empty class first."""
    f32 = np.float32
    wt = [f32(n) * f32(w) if n > 0 else f32(0) for n, w in zip(counts, cw)]
    tot = f32(0)
    for x in wt:
        tot = f32(tot + x)
    nonempty = sum(n > 0 for n in counts)
    assert 0 < nonempty <= units, 'the class schedule needs a unit per non-empty class'
    wc, fr = [], []
    for x in wt:
        v = f32(units - nonempty) * f32(x / tot) if x > 0 else f32(0)
        fl = int(v)
        wc.append(1 + fl if x > 0 else 0)
        fr.append(float(v) - fl)
    for _ in range(units - sum(wc)):
        best = max((c for c in range(4) if wt[c] > 0), key=lambda c: (fr[c], -c))
        wc[best] += 1
        fr[best] = -2.0
    return wc


def restate(counts, cus, bwd):
    """For every grid the launch may have: per class, the waves it gets and the pairs per
    wave q, with q's range should the class's unit count be one more or one less (the
    device may round the float shares otherwise than numpy does).  At 8 waves per block a
    CU holds 1 block (backward) or 2 (forward); at fewer waves the count depends on LDS
    sizes this restatement does not know, so every possible count is listed."""
    nw = waves_per_block()
    n = int(sum(counts))
    wcap = 8 if bwd else 16
    per_cus = [wcap // nw] if nw == 8 else list(range(1, wcap // nw + 1))
    cw = class_weights(bwd)
    out, seen = [], set()
    for per_cu in per_cus:
        blocks = min(max((n + nw - 1) // nw, 1), cus * per_cu)
        if blocks in seen:
            continue
        seen.add(blocks)
        align = nw == 8
        units = blocks * nw // 2 if align else blocks * nw
        u = unit_counts(counts, cw, units)
        per = 2 if align else 1
        cls, cum = [], 0
        for c in range(4):
            if counts[c] == 0:
                cls.append(None)
                continue
            qs = [counts[c] // (per * k) for k in (u[c] + 1, u[c], u[c] - 1) if k >= 1]
            cls.append(dict(waves=per * u[c], first=cum, q=counts[c] // (per * u[c]),
                            q_lo=min(qs), q_hi=max(qs)))
            cum += per * u[c]
        out.append(dict(blocks=blocks, waves_per_block=nw, cls=cls))
    return out


def assert_reaches(spec, counts, cus):
    """The case's `many` class has q >= 64 and every other class q < 64, forward and
    backward, on every possible grid, also with a unit more or less."""
    res = {}
    for name, bwd in (('fwd', False), ('bwd', True)):
        res[name] = restate(counts, cus, bwd)
        for g in res[name]:
            for c, k in enumerate(g['cls']):
                if k is None:
                    continue
                if c == spec.get('many'):
                    assert k['q_lo'] >= Q_MANY, (spec['name'], name, c, g)
                    if spec.get('two_blocks'):   # k runs past one block's 8 positions
                        last = k['first'] + k['waves'] - 1
                        assert (k['first'] >> 3) != (last >> 3), (spec['name'], name, c, g)
                    elif spec.get('one_unit'):
                        assert k['waves'] == (2 if g['waves_per_block'] == 8 else 1), g
                else:
                    assert k['q_hi'] < Q_MANY, (spec['name'], name, c, g)
    return res


# ---- cases: pairs per class (class = (N0 > 8) + 2 (N1 > 8)) ----
def _case(name, counts, seed, **kw):
    return dict(name=name, counts=list(counts), seed=seed, **kw)


CASES = {c['name']: c for c in [
    # few pairs per wave (branch 1 at 8 waves per block, branch 2 below)
    _case('only0', (30, 0, 0, 0), 101),
    _case('only1', (0, 30, 0, 0), 102),
    _case('only2', (0, 0, 30, 0), 103),
    _case('only3', (0, 0, 0, 30), 104),
    _case('single_pair_class', (0, 1, 38, 0), 105),
    _case('four_4', (1, 1, 1, 1), 106),       # one block; a unit per class and none over
    _case('four_5', (2, 1, 1, 1), 111),       # two blocks at 4 and at 3 waves per block
    _case('four_9', (3, 2, 2, 2), 107),       # two blocks
    _case('four_2049', (600, 500, 500, 449), 108),   # just over a pair per wave (256 blocks)
    # record 0 in the last class of the order, the last record in its first class
    _case('ends_differ', (20, 0, 0, 17), 109, first=3, last=0),
    # many pairs per wave in one class (branches 3 and 4), under skewed SG_CLS_W
    _case('skew_one', (600, 1000, 600, 600), 201, many=1, one_unit=True),
    _case('skew_one_small', (50, 300, 7, 1), 202, many=1, one_unit=True),
    _case('skew_two_blocks', (350, 350, 2000, 300), 203, many=2, two_blocks=True),
]}
CLS_W_ONE = '1,1e-6,1,1'          # class 1 keeps the one unit every non-empty class gets
CLS_W_TWO = '1,1,0.003525,1'      # class 2 of skew_two_blocks: 0.7% of the units


def build_case(spec):
    """small_problem with the pairs redrawn so that `counts[c]` of them have class c, in
    shuffled order (optionally with the first and the last record's class fixed)."""
    counts = spec['counts']
    n = int(sum(counts))
    assert 0 < n <= MAX_PAIRS
    prob = small_problem(n_graphs=40, n_pairs=n, seed=spec['seed'], n_lo=3, n_hi=10)
    rng = np.random.default_rng(spec['seed'] + 7)
    nodes = np.array([g.number_of_nodes() for g in prob.graphs])
    small, big = np.flatnonzero(nodes <= 8), np.flatnonzero(nodes > 8)
    assert len(small) > 1 and len(big) > 1
    cls = np.repeat(np.arange(4), counts)
    rng.shuffle(cls)
    for pos, key in ((0, 'first'), (n - 1, 'last')):
        if key in spec:
            j = int(np.flatnonzero(cls == spec[key])[0 if pos else -1])
            cls[pos], cls[j] = cls[j], cls[pos]
    for side in (0, 1):
        is_big = (cls >> side) & 1
        prob.pairs[:, side] = np.where(is_big, rng.choice(big, n), rng.choice(small, n))
    prob.labels[:] = LABEL
    assert np.array_equal(np.bincount(cls, minlength=4), counts)
    return prob, cls


# ---- witnesses ----
def _rel(g, g_ref, prob):
    """check_grad_per_var's per-variable metric, without its assertion."""
    return check_grad_per_var(g, g_ref, prob.layers, prob.d_in, tol=float('inf'))


def run_case(spec, device):
    import torch
    from graphembedding_amd import _lib
    t0 = time.time()
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    reach = assert_reaches(spec, spec['counts'], cus)
    prob, cls = build_case(spec)
    model, batch = prob.make_gpu_model(device=device)
    assert model.kernel_path == 1 and model.n_max == 10 and prob.flags.dropout == 0.1
    n = batch.n_pairs
    keep = []   # every score buffer stays allocated: none is handed out twice

    def nan_buf(k):
        keep.append(torch.full((k,), float('nan'), dtype=torch.float32, device=device))
        return keep[-1]

    def forward(b):
        s = nan_buf(b.n_pairs)
        _lib.forward(model.sg, b.records, b.n_pairs, b.pair_offset, model.params, SEED, s,
                     order=b.order, class_start=b.cls)
        return s.cpu().numpy()

    def step(b):
        # without the label term (a constant of y_stats): the loss is the pairs' own sum
        s = nan_buf(b.n_pairs)
        model.fwd_bwd(b, seed=SEED, s_out=s, add_label_term=False)
        return (s.cpu().numpy(), model.grad.cpu().numpy().astype(np.float64),
                float(model.loss_buf[0].item()))

    model.balance(batch, classes=False)
    assert batch.cls is None and batch.order is not None
    s_mix = forward(batch)
    sb_mix, g_mix, l_mix = step(batch)
    model.balance(batch, classes=True)
    table = batch.cls.cpu().tolist()
    s_cls = forward(batch)
    sb_cls, g_cls, l_cls = step(batch)
    _, g_again, _ = step(batch)
    rel = _rel(g_cls, g_mix, prob)
    r = dict(case=spec['name'], n_pairs=n, counts=spec['counts'], class_table=table,
             reach=reach,
             mix_nan=int(np.isnan(s_mix).sum() + np.isnan(sb_mix).sum()),
             mix_fwd_eq_bwd=bool(np.array_equal(s_mix, sb_mix)),
             fwd_nan=int(np.isnan(s_cls).sum()), fwd_equal=bool(np.array_equal(s_cls, s_mix)),
             bwd_nan=int(np.isnan(sb_cls).sum()), bwd_equal=bool(np.array_equal(sb_cls, s_mix)),
             grad_rel=max(rel.values()), grad_rel_var=max(rel, key=rel.get),
             loss_rel=abs(l_cls - l_mix) / abs(l_mix),
             replay_equal=bool(np.array_equal(g_cls, g_again)), guard={}, oracle=None)

    # sensitivity guard: the batch without the last pair of class c, as the records before
    # it plus the records after it at their own pair offset (every other pair keeps its
    # dropout key), on the mixed schedule
    W = batch.records.numel() // n
    for c in range(4):
        if spec['counts'][c] == 0:
            continue
        i = int(np.flatnonzero(cls == c)[-1])
        g_drop, l_drop = np.zeros_like(g_mix), 0.0
        for lo, hi in ((0, i), (i + 1, n)):
            if hi == lo:
                continue
            b = model.batch_from_records(batch.records[lo * W:hi * W], hi - lo,
                                         batch.labels[lo:hi], lo, n, y_stats=batch.y_stats)
            model.balance(b, classes=False)
            _, g, l = step(b)
            g_drop += g
            l_drop += l
        rel = _rel(g_drop, g_mix, prob)
        r['guard'][str(c)] = dict(record=i, grad_rel=max(rel.values()),
                                  loss_rel=abs(l_drop - l_mix) / abs(l_mix))

    if n <= ORACLE_PAIRS:
        ref = run_oracle_step(prob, SEED, adam=False)
        rel = _rel(g_cls, ref.grad_mse, prob)
        r['oracle'] = dict(
            score_err=float(np.max(np.abs(s_cls - ref.s) / (1.0 + np.abs(ref.s)))),
            grad_rel=max(rel.values()))
    r['seconds'] = round(time.time() - t0, 3)
    return r


def check_result(r):
    """Every assertion on one case's figures (printed first: pytest shows them on failure)."""
    print(json.dumps(r))
    n = r['n_pairs']
    assert r['class_table'] == np.concatenate([[0], np.cumsum(r['counts'])]).tolist()
    assert r['mix_nan'] == 0 and r['mix_fwd_eq_bwd'], 'mixed schedule: skipped or moved slot'
    assert r['fwd_nan'] == 0, 'class schedule, forward: {} of {} slots skipped'.format(
        r['fwd_nan'], n)
    assert r['fwd_equal'], 'class schedule, forward: scores differ from the mixed schedule'
    assert r['bwd_nan'] == 0, 'class schedule, backward: {} of {} slots skipped'.format(
        r['bwd_nan'], n)
    assert r['bwd_equal'], 'class schedule, backward: scores differ from the mixed schedule'
    assert r['grad_rel'] <= TOL, (r['grad_rel_var'], r['grad_rel'])
    assert r['loss_rel'] <= TOL, r['loss_rel']
    assert r['replay_equal'], 'class-schedule fwd_bwd is not bitwise reproducible'
    assert sorted(r['guard']) == [str(c) for c in range(4) if r['counts'][c] > 0]
    for c, g in r['guard'].items():
        assert g['grad_rel'] >= 10 * TOL, ('one lost pair of class', c, 'would pass', g)
        assert g['loss_rel'] >= 10 * TOL, ('one lost pair of class', c, 'would pass', g)
    if n <= ORACLE_PAIRS:
        assert r['oracle']['score_err'] <= ORACLE_TOL, r['oracle']
        assert r['oracle']['grad_rel'] <= ORACLE_TOL, r['oracle']


def main(names):
    import torch
    assert torch.cuda.is_available(), 'no HIP device is visible'
    device = torch.device('cuda:0')
    torch.zeros(1, device=device).item()
    from graphembedding_amd import _lib
    _lib.lib()
    startup = round(time.time() - T_START, 3)   # interpreter, torch, HIP and library start-up
    out = dict(startup_seconds=startup, waves_per_block=waves_per_block(),
               cus=torch.cuda.get_device_properties(device).multi_processor_count,
               env={k: os.environ.get(k) for k in ('SG_CLS_W', 'SG_XCD_W', 'SG_FAST_WAVES')},
               cases=[run_case(CASES[k], device) for k in names])
    torch.cuda.synchronize()
    out['total_seconds'] = round(time.time() - T_START, 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1:])
