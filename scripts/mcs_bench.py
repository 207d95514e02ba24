"""The budgeted MCS search (include/siamese_mcs.h) on the AIDS700nef-shaped grid (GPU only).

    python scripts/mcs_bench.py [--repeats 5] [--budget 1048576] [--sample 40] [--out FILE.json]

One grid: syn_aids700nef, 700 x 700 = 490,000 pairs of 5 .. 10 nodes, capacity 10, one
sg_mcs_grid call (two launches) per `connected` value at the default budget of 2^20 expansions
per pair, with bound_out and expansions_out and no map.  Device times are HIP events around the
call with every buffer allocated beforehand, after one warm-up call of each; the repeats
alternate between the two `connected` values so a drift of the clocks falls on both; median
with min .. max.

Recorded besides the times: pairs/s, expansions/s, the share of pairs proven (size == bound),
the histogram of expansions per pair by powers of two, the largest count and the sum, the mean
size, and the kernel's scratch and LDS bytes as the compiler reports them for the product
build's options.  Before timing, --sample random pairs must equal the restatement
(tests/_mcs_restatement.py) in size, bound and expansions.  Prints one JSON line; by default it
is also written to profiles/mcs/mcs_bench.json.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _arg(name, default):
    a = sys.argv[1:]
    return type(default)(a[a.index(name) + 1]) if name in a else default


class Grid(object):
    """The all-pairs grid with its buffers; run() is the bare C-ABI call."""

    def __init__(self, store, device, connected, budget):
        import torch
        from graphembedding_amd import _lib
        self._lib, self.store, self.connected, self.budget = _lib, store, connected, budget
        self.dev = store.to_device(device)
        self.G = G = len(store)
        nbytes = _lib.mcs_grid_workspace_bytes(G, G, store.n_max)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        self.size = torch.empty((G, G), dtype=torch.int32, device=device)
        self.bound = torch.empty((G, G), dtype=torch.int32, device=device)
        self.ex = torch.empty((G, G), dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self):
        self._lib.mcs_grid(self.dev, self.store.n_max, None, self.G, None, self.G,
                           self.connected, self.budget, self.size, self.G, self.bound, None,
                           None, self.ex, self.status, self.ws)

    def timed(self):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)


def kernel_resources():
    """(scratch bytes per lane, LDS bytes per workgroup) of sg_mcs_kernel from the code object
    metadata of a device-only compile with the product build's options, or (None, None)."""
    from graphembedding_amd import build as B
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    with tempfile.TemporaryDirectory(prefix='sg_mcs_') as tmp:
        dst = os.path.join(tmp, 'sg_mcs.s')
        cmd = [hipcc, '--offload-arch=' + B.ARCH, '-O3', '-std=c++17', '-fPIC',
               '-fno-slp-vectorize', '--cuda-device-only', '-S', '-w'] + \
            B.SOURCE_FLAGS.get('sg_mcs.hip', []) + [os.path.join(B.CSRC, 'sg_mcs.hip'), '-o', dst]
        try:
            subprocess.run(cmd, cwd=B.CSRC, check=True, capture_output=True)
            text = open(dst).read()
        except (OSError, subprocess.CalledProcessError):
            return None, None
    # the metadata entry of the kernel: its fields come in alphabetical order
    mt = re.search(r'\.group_segment_fixed_size:\s*(\d+)(?:(?!\.group_segment_fixed_size).)*?'
                   r'\.name:\s*\S*sg_mcs_kernel\S*.*?\.private_segment_fixed_size:\s*(\d+)',
                   text, re.S)
    return (int(mt.group(2)), int(mt.group(1))) if mt else (None, None)


def _stats(ms, pairs, expansions):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return dict(ms_median=med, ms_min=ms[0], ms_max=ms[-1], repeats=len(ms),
                pairs_per_s=pairs / (med * 1e-3), expansions_per_s=expansions / (med * 1e-3))


def main():
    import torch
    from graphembedding_amd.allpairs import load_graph_set
    from graphembedding_amd.build import build_hip
    from graphembedding_amd.mcs import MCS_DEFAULT_BUDGET
    build_hip()
    device = torch.device('cuda:0')
    repeats, n_sample = _arg('--repeats', 5), _arg('--sample', 40)
    budget = _arg('--budget', MCS_DEFAULT_BUDGET)
    store = load_graph_set('syn_aids700nef').store
    grids = [Grid(store, device, c, budget) for c in (False, True)]
    for g in grids:   # warm-up
        g.run()
    torch.cuda.synchronize()
    times = [[], []]
    for _ in range(repeats):
        for k, g in enumerate(grids):
            times[k].append(g.timed())
    import _mcs_restatement as X
    ref = X.McsGridReference(store)
    rng = np.random.default_rng(0)
    G = grids[0].G
    n = np.asarray(store.n)
    scratch, lds = kernel_resources()
    result = dict(bench='mcs_grid', gpu=torch.cuda.get_device_name(0), grid='aids700nef',
                  graphs=G, pairs=G * G, n_max=store.n_max, nodes_min=int(n.min()),
                  nodes_max=int(n.max()), budget=budget,
                  packing='one pair per wavefront, one lane per class part',
                  kernel_scratch_bytes_per_lane=scratch, kernel_lds_bytes_per_workgroup=lds)
    for k, g in enumerate(grids):
        assert int(g.status.item()) == 0
        size, bound, ex = (t.cpu().numpy() for t in (g.size, g.bound, g.ex))
        assert (size <= bound).all() and (size >= 0).all() and (ex <= budget).all()
        assert np.array_equal(np.diag(size), n[:G])
        proven = size == bound
        cand = np.argwhere(ex <= 5000)   # cheap ones: the host is slow
        sample = cand[rng.permutation(len(cand))[:n_sample]]
        for a, b in sample:
            want = ref.pair(int(a), int(b), g.connected, budget)
            assert (want[0], want[1], want[4]) == \
                (int(size[a, b]), int(bound[a, b]), int(ex[a, b])), (a, b)
        bins = np.zeros(26, dtype=np.int64)   # bin i: 2^(i-1) <= expansions < 2^i; bin 0: none
        np.add.at(bins, np.where(ex > 0, np.floor(np.log2(np.maximum(ex, 1))).astype(np.int64) + 1,
                                 0), 1)
        result['connected' if g.connected else 'unconnected'] = dict(
            _stats(times[k], G * G, int(ex.sum())), proven_share=float(proven.mean()),
            proven_pairs=int(proven.sum()), unproven_pairs=int((~proven).sum()),
            expansions_histogram_pow2=bins.tolist(), expansions_max=int(ex.max()),
            expansions_sum=int(ex.sum()), expansions_mean=float(ex.mean()),
            size_mean=float(size.mean()), bound_mean=float(bound.mean()),
            checked_against_restatement=int(len(sample)))
    line = json.dumps(result)
    print(line)
    out = _arg('--out', os.path.join(ROOT, 'profiles', 'mcs', 'mcs_bench.json'))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
