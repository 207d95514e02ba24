"""The fused kernel's class-exclusive wave schedule (sg_fast.hip, "pair schedule"), on every
branch of its slot split: the ranges [cs0, cs1) of all waves must tile the order exactly
once.  A slot no wave takes is a pair that never trains, a slot taken twice a pair counted
twice; both give plausible numbers, so each case (tests/_schedule_child.py) looks for both:

  skips     forward (sg_forward_cls) and backward (sg_fwd_bwd_cls) write their scores into
            NaN-filled buffers: no NaN may remain, and the scores equal the mixed
            schedule's bit for bit (the mixed schedule is held to the oracle by
            test_gpu_parity and test_gpu_order; cases of <= 40 pairs are held to it here)
  repeats   the gradient equals the mixed schedule's per variable (check_grad_per_var) and
            the loss relative to itself, within the 1e-5 of a reassociated fp32 sum over
            <= 4096 pairs (test_large_batch_properties); every case has <= 4096 pairs
  guard     for each non-empty class, the mixed-schedule step WITHOUT one pair of that
            class differs from the full one by >= 10 x that tolerance in a variable's
            gradient and in the loss: one lost (or doubled) pair cannot pass
  replay    a second class-scheduled step gives the same gradient bitwise

The branch is chosen in the kernel by q = pairs per wave of a class, the waves per block
and the XCD weights.  SG_CLS_W, SG_XCD_W and SG_FAST_WAVES are read once per process (and
SG_FAST_WAVES sizes workspaces), so every setting runs in a child process of its own, one
after another.  The child restates the wave split (classes -> units -> q) to assert, with
a margin of one unit either way, that the case reaches its branch; the restatement is
never a reference for results.

Branches reached, forward (F) and backward (B), with q of the targeted class as restated
on an MI355X (256 CUs; at 8 waves per block the backward grid has 256 blocks, the forward
grid two per CU; below 8 waves per block q is listed for every grid the launch may have):

  1  q < 64, 8 waves per block.  F and B: every in-process case (q <= 1; four_2049 has
     q = 1 or 0 plus remainders on 256 blocks B, 257 blocks F), and the three untargeted
     classes of every skewed case at 8 waves per block (q = 0, remainders only)
  2  q < 64, fewer waves per block (old_below).  F and B: waves4 (four_2049 q = 2, 1 or 0
     on 256, 512 or 513 blocks; the small cases q <= 1) and waves3 (four_2049 q = 3 ... 0
     on 256, 512 or 683 blocks); four_4 at 4 waves per block has a unit per class and none
     over; also the untargeted classes of the skewed cases below 8 waves per block
  3  q >= 64, equal XCD weights.  cls_one: skew_one q = 500 and skew_one_small q = 150, F
     and B, 2 waves (one unit).  cls_two: skew_two_blocks B q = 125 (16 waves from position
     1422), F q = 90 (22 waves from position 2084).  Without `align`: waves4_cls_two
     (q = 250, 133 or 90 on 8, 15 or 22 waves), waves3_cls_one (q = 300, one wave)
  4  q >= 64, unequal XCD weights (F(x)).  cls_one_xcd, cls_two_xcd and cls_two_xcd_spread:
     the cases and q of branch 3.  Without `align`: waves3_cls_two_xcd (q = 333, 166, 117
     or 90 on 6, 12, 17 or 22 waves), waves4_cls_one_xcd_spread (q = 300, one wave)

Not covered: the 64-bit variant of branch 3 needs count x waves >= 2^32 for one class,
millions of pairs."""
import json
import os
import subprocess
import sys

import pytest

import _schedule_child as sc

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_schedule_child.py')
# A child took 2.2 to 2.6 s on an MI355X box, of which 1.9 to 2.3 s interpreter, torch, HIP
# and library start-up (a case itself runs 0.01 to 0.15 s); the limit is a few times that.
CHILD_TIMEOUT = 20

XCD_NEAR = '10000,10400,9600,10900,9100,10700,9300,10200'   # within 10% of the default
XCD_SPREAD = '1,30000,10000,1,30000,10000,1,30000'          # pushes F's integer quotients
FEW = ['four_4', 'four_5', 'four_9', 'four_2049', 'only3', 'single_pair_class']

IN_PROCESS = ['only0', 'only1', 'only2', 'only3', 'single_pair_class', 'four_4', 'four_9',
              'four_2049', 'ends_differ']

CHILDREN = {
    'cls_one': (dict(SG_CLS_W=sc.CLS_W_ONE), ['skew_one', 'skew_one_small']),
    'cls_two': (dict(SG_CLS_W=sc.CLS_W_TWO), ['skew_two_blocks']),
    'cls_one_xcd': (dict(SG_CLS_W=sc.CLS_W_ONE, SG_XCD_W=XCD_NEAR),
                    ['skew_one', 'skew_one_small']),
    'cls_two_xcd': (dict(SG_CLS_W=sc.CLS_W_TWO, SG_XCD_W=XCD_NEAR), ['skew_two_blocks']),
    'cls_two_xcd_spread': (dict(SG_CLS_W=sc.CLS_W_TWO, SG_XCD_W=XCD_SPREAD),
                           ['skew_two_blocks']),
    'waves4': (dict(SG_FAST_WAVES='4'), FEW),
    'waves3': (dict(SG_FAST_WAVES='3'), FEW),
    'waves4_cls_two': (dict(SG_FAST_WAVES='4', SG_CLS_W=sc.CLS_W_TWO), ['skew_two_blocks']),
    'waves3_cls_one': (dict(SG_FAST_WAVES='3', SG_CLS_W=sc.CLS_W_ONE), ['skew_one_small']),
    'waves3_cls_two_xcd': (dict(SG_FAST_WAVES='3', SG_CLS_W=sc.CLS_W_TWO, SG_XCD_W=XCD_NEAR),
                           ['skew_two_blocks']),
    'waves4_cls_one_xcd_spread': (dict(SG_FAST_WAVES='4', SG_CLS_W=sc.CLS_W_ONE,
                                       SG_XCD_W=XCD_SPREAD), ['skew_one_small']),
}

_child_died = []   # a child ended by signal or time limit: no later test starts another


def run_child(env_extra, cases):
    """One child under the given settings; its parsed JSON line.  A child that ends by
    signal, time limit or failure fails the calling test."""
    if _child_died:
        pytest.fail('not started: an earlier child ended by {}'.format(_child_died[0]))
    env = {k: v for k, v in os.environ.items()
           if k not in ('SG_CLS_W', 'SG_XCD_W', 'SG_FAST_WAVES', 'SG_DISABLE_FAST')}
    env.update(env_extra)
    try:
        p = subprocess.run([sys.executable, CHILD] + list(cases), env=env, text=True,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_died.append('its time limit')
        raise
    if p.returncode < 0:
        _child_died.append('signal {}'.format(-p.returncode))
    assert p.returncode == 0, 'child exit status {}\n{}'.format(p.returncode, p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert lines, p.stdout[-2000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize('name', IN_PROCESS)
def test_class_schedule_default_settings(gpu, name):
    """Few pairs per wave at 8 waves per block (branch 1), in this process."""
    for k in ('SG_CLS_W', 'SG_XCD_W', 'SG_FAST_WAVES'):
        assert k not in os.environ, k
    sc.check_result(sc.run_case(sc.CASES[name], gpu))


@pytest.mark.parametrize('name', list(CHILDREN))
def test_class_schedule_in_child(gpu, name):
    """Branches 2, 3 and 4 (module docstring), each setting in a fresh process."""
    env, cases = CHILDREN[name]
    out = run_child(env, cases)
    print(json.dumps({k: v for k, v in out.items() if k != 'cases'}))
    assert out['env'] == {k: env.get(k) for k in ('SG_CLS_W', 'SG_XCD_W', 'SG_FAST_WAVES')}
    assert [r['case'] for r in out['cases']] == cases
    for r in out['cases']:
        sc.check_result(r)
