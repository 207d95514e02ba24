"""Embed-once training with graph-keyed dropout on the GPU (include/siamese_embed_drop.h):
sg_embed_drop against the oracle's _node_forward and head mask, against the masks the pair
kernels draw, its independence of partner and call split, sg_embed_drop_bwd and
grid_fwd_bwd(dropout='graph') against a float64 reference built from oracle pieces, invalid
entries, and the Python surface.
Bars are imported, not restated: embeddings and scores within test_gpu_embed.TOL (rtol =
atol), loss and every gradient block within test_gpu_embed_train.TOL of its own largest
component.  The 1 / keep <= 2 scaling of the masked tensors does not change their order."""
import numpy as np
import pytest

from _embed_fixtures import ATTENTION_STACK, gpu_model, oracle_graphs, sized_problem
from _fixtures import AVERAGE_STACK, check_grad_per_var
from oracle import siamese_oracle as O
from test_gpu_embed import TOL as EMBED_TOL
from test_gpu_embed_train import TOL as TRAIN_TOL
from test_gpu_embed_train import _autograd_head, _block_close, _offsets

pytestmark = pytest.mark.gpu

STACKS = {'default': {}, 'average': AVERAGE_STACK, 'attention': ATTENTION_STACK}
KEEPS = (0.5, 0.9)
N_GRAPHS = 70
SEED = 0x1234_5678_9ABC


def _counts():
    """1, 8, 9 and the Padding dim first, then random node counts."""
    rng = np.random.default_rng(3)
    return [1, 8, 9, 10] + [int(x) for x in rng.integers(1, 11, size=N_GRAPHS - 4)]


_CASES = {}


def _case(stack, keep, gpu):
    """Problem, model, store and its device copy of a stack at a keep probability: built
    once, read only."""
    key = (stack, keep)
    if key not in _CASES:
        from graphembedding_amd.packer import GraphStore
        ov = dict(STACKS[stack], dropout=round(1.0 - keep, 6), node_feat_order='sorted')
        prob = sized_problem(_counts(), ov, n_max=10, seed=11)
        model = gpu_model(prob, gpu)
        store = GraphStore(prob.mgs, model.n_max, prob.d_in)
        _CASES[key] = (prob, model, store, store.to_device(gpu))
    return _CASES[key]


def _embed_drop(model, dev, idx, seed, entry_offset=0, sg=None):
    """sg_embed_drop into a sentinel-filled buffer: (rows [count][E] torch, status)."""
    import torch
    from graphembedding_amd import _lib
    gpu = model.params.device
    idx_t = torch.as_tensor(np.asarray(idx), dtype=torch.int32, device=gpu)
    out = torch.full((len(idx), model.embed_dim), 7.0, dtype=torch.float32, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    _lib.embed_drop(sg or model.sg, dev, model.n_max, idx_t, len(idx), entry_offset,
                    model.params, seed, out, status)
    torch.cuda.synchronize()
    return out, int(status.item())


def _embed_drop_bwd(model, dev, idx, seed, g_emb, entry_offset=0):
    """sg_embed_drop_bwd: (grad_out with a sentinel in the head range, status)."""
    import torch
    from graphembedding_amd import _lib
    from test_gpu_embed_train import SENTINEL
    gpu = model.params.device
    idx_t = torch.as_tensor(np.asarray(idx), dtype=torch.int32, device=gpu)
    grad = torch.full((model.n_params,), SENTINEL, dtype=torch.float32, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(_lib.embed_drop_bwd_workspace_bytes(model.sg, len(idx)) // 4 + 1,
                     dtype=torch.float32, device=gpu)
    _lib.embed_drop_bwd(model.sg, dev, model.n_max, idx_t, len(idx), entry_offset, model.params,
                        seed, torch.from_numpy(np.ascontiguousarray(g_emb, np.float32)).to(gpu),
                        grad, ws, status)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), int(status.item())


class _Oracle:
    """The contract in oracle terms: entry c' is side c' & 1 of pair c' >> 1."""

    def __init__(self, prob):
        self.spec = prob.oracle_spec()
        self.P = O.unflatten(self.spec, prob.params.astype(np.float64))
        self.gs = oracle_graphs(prob)
        self.hi = O._head_index(self.spec)
        head = self.spec.layers[self.hi]
        self.keep = self.spec.layer_keep(head) if head['kind'] == 'NTN' else 1.0

    def entry(self, gi, c, seed):
        """(masked embedding [E], head mask, caches, shape of the stack's output)."""
        x, caches = O._node_forward(self.spec, self.P, self.gs[gi], c & 1, c >> 1, seed)
        e = np.asarray(x, np.float64).reshape(-1)
        m = O.dropout_mask(seed, c >> 1, c & 1, self.hi, e.size, self.keep)
        return np.where(m, e / self.keep, 0.0), m, caches, np.shape(x)

    def rows(self, idx, seed, entry_offset=0):
        return np.stack([self.entry(gi, entry_offset + c, seed)[0] for c, gi in enumerate(idx)])


# ---- 1. forward against the oracle -------------------------------------------------------
@pytest.mark.parametrize('count', [5, 65])   # an odd tail each; 65: 33 units, > one workgroup
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('stack', list(STACKS))
def test_embed_drop_matches_oracle(gpu, stack, keep, count):
    prob, model, store, dev = _case(stack, keep, gpu)
    assert abs(model.sg.keep_prob - keep) < 1e-6
    idx = np.random.default_rng(count).permutation(N_GRAPHS)[:count]
    idx[:4] = [3, 0, 2, 1]                     # node counts 10, 1, 9, 8
    got, st = _embed_drop(model, dev, idx, SEED)
    assert st == 0
    want = _Oracle(prob).rows(idx, SEED)
    got = got.cpu().numpy()
    dropped = float((want == 0).mean())
    print(stack, keep, count, 'max |emb - oracle|', float(np.abs(got - want).max()),
          'zeros', dropped)
    # the head mask bites: of 65 x 16 pooled values a fraction 1 - keep is zero, within five
    # binomial standard deviations (0.016 at keep 0.5); the default stack's relu and padding
    # rows are zero anyway
    if stack != 'default' and count == 65:
        assert abs(dropped - (1 - keep)) < 0.08
    np.testing.assert_allclose(got, want, rtol=EMBED_TOL, atol=EMBED_TOL)


# ---- 2. the masks of the pair kernel -----------------------------------------------------
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('stack', list(STACKS))
def test_embed_drop_draws_the_pair_kernels_masks(gpu, stack, keep):
    """Pair q = (g_2q, g_2q+1) through model.pred_sim_without_act (dropout on, pair_offset 0)
    against grid entry (2 q, 2 q + 1) of the masked embeddings under the same seed."""
    import torch
    from graphembedding_amd import _lib
    from graphembedding_amd.packer import pack_device
    prob, model, store, dev = _case(stack, keep, gpu)
    npair = 8
    ids = np.array([3, 0, 2, 1] + list(range(20, 32)))
    pairs = ids.reshape(npair, 2).astype(np.int32)
    recs, status = pack_device(store, pairs, None, device=gpu, dtype=model.record_dtype)
    batch = model.batch_from_records(recs, npair, np.zeros(npair, np.float32))
    assert batch.pair_offset == 0
    fwd = model.pred_sim_without_act(batch, seed=SEED).cpu().numpy().reshape(-1)
    assert int(status.item()) == 0
    emb, st = _embed_drop(model, dev, ids, SEED)
    assert st == 0
    keep1 = model._sg_keep1()
    assert keep1.keep_prob == 1.0 and abs(model.sg.keep_prob - keep) < 1e-6
    n = 2 * npair
    ws = torch.empty(_lib.score_grid_workspace_bytes(keep1, n) // 4 + 1, dtype=torch.float32,
                     device=gpu)
    out = torch.empty((n, n), dtype=torch.float32, device=gpu)
    _lib.score_grid(keep1, emb, emb, n, n, model.params, False, out, n, ws)
    out = out.cpu().numpy()
    got = np.array([out[2 * q, 2 * q + 1] for q in range(npair)])
    plain = model.pred_sim_without_act(batch, seed=SEED + 1).cpu().numpy().reshape(-1)
    print(stack, keep, 'kernel path', model.kernel_path, 'max |grid - pair|',
          float(np.abs(got - fwd).max()), 'other seed', float(np.abs(plain - fwd).max()))
    assert np.abs(plain - fwd).max() > 10 * EMBED_TOL     # the masks matter to these scores
    np.testing.assert_allclose(got, fwd, rtol=EMBED_TOL, atol=EMBED_TOL)


# ---- 3. partner independence -------------------------------------------------------------
@pytest.mark.parametrize('stack', list(STACKS))
def test_embed_drop_rows_do_not_depend_on_partner_or_split(gpu, stack):
    import torch
    prob, model, store, dev = _case(stack, 0.5, gpu)
    idx = np.array([3, 0, 2, 1, 20, 21, 22, 23, 24])   # nine entries: an odd tail
    whole, st = _embed_drop(model, dev, idx, SEED)
    assert st == 0
    other = idx.copy()
    other[1::2] = [40, 41, 3, 43]                       # every side-1 partner replaced
    a, _ = _embed_drop(model, dev, other, SEED)
    assert torch.equal(a[0::2], whole[0::2])
    assert not torch.equal(a[1], whole[1])
    other = idx.copy()
    other[0::2] = [50, 51, 1, 53, 54]                   # every side-0 partner replaced
    b, _ = _embed_drop(model, dev, other, SEED)
    assert torch.equal(b[1::2], whole[1::2])
    # a call split at an even boundary
    tail, st = _embed_drop(model, dev, idx[4:], SEED, entry_offset=4)
    assert st == 0 and torch.equal(tail, whole[4:])
    mid, _ = _embed_drop(model, dev, idx[4:8], SEED, entry_offset=4)
    assert torch.equal(mid, whole[4:8])
    # the entry number counts, not the position in the call
    shifted, _ = _embed_drop(model, dev, idx[4:], SEED, entry_offset=0)
    assert not torch.equal(shifted, whole[4:])


# ---- 4. seed and keep --------------------------------------------------------------------
@pytest.mark.parametrize('stack', list(STACKS))
def test_embed_drop_seed_and_keep_one(gpu, stack):
    import torch
    from graphembedding_amd import _lib
    from test_gpu_embed_train import _run_embed_bwd
    prob, model, store, dev = _case(stack, 0.5, gpu)
    idx = np.random.default_rng(4).permutation(N_GRAPHS)[:9]
    a, _ = _embed_drop(model, dev, idx, SEED)
    b, _ = _embed_drop(model, dev, idx, SEED + 1)
    again, _ = _embed_drop(model, dev, idx, SEED)
    assert torch.equal(a, again) and not torch.equal(a, b)
    # keep_prob = 1: sg_embed, bit for bit, whatever the seed and the offset
    plain = gpu_model(prob, gpu, dropout=0.0)
    assert plain.sg.keep_prob == 1.0
    idx_t = torch.as_tensor(idx, dtype=torch.int32, device=gpu)
    ref = torch.empty((len(idx), plain.embed_dim), dtype=torch.float32, device=gpu)
    _lib.embed(plain.sg, dev, plain.n_max, idx_t, len(idx), plain.params, ref, None)
    for seed, off in ((SEED, 0), (SEED + 1, 6)):
        got, st = _embed_drop(plain, dev, idx, seed, entry_offset=off)
        assert st == 0 and torch.equal(got, ref)
    # ... and sg_embed_drop_bwd is sg_embed_bwd up to the summation order of its LDS atomics
    g_emb = np.random.default_rng(5).standard_normal((len(idx), plain.embed_dim)).astype(np.float32)
    want, st = _run_embed_bwd(plain, dev, idx, g_emb)
    assert st == 0
    got, st = _embed_drop_bwd(plain, dev, idx, SEED, g_emb)
    assert st == 0
    _node_blocks_close(prob, got, want)


def _node_blocks_close(prob, got, want):
    """Every node-layer variable within TRAIN_TOL of its own largest component; the head's
    range of grad_out untouched."""
    from test_gpu_embed_train import SENTINEL
    offs, total = _offsets(prob)
    hi = len(prob.layers) - 1
    head0 = offs[(hi, 'weights_W')][0]
    assert np.all(got[head0:] == SENTINEL), 'the head range of grad_out was written'
    for (li, name), (o, shape) in offs.items():
        if li != hi:
            n = int(np.prod(shape))
            _block_close(got[o:o + n], want[o:o + n], '{}.{}'.format(li, name))


# ---- 5. the gradient against a float64 reference -----------------------------------------
def _reference_step(prob, q, db, labels, seed):
    """Loss and flat gradient of grid_fwd_bwd(dropout='graph') in float64: per distinct graph
    the oracle's _node_forward under its entry's masks and the head mask; the NTN head, loss
    and adjoint over the m x n block at keep 1 (test_gpu_embed_train._autograd_head) on the
    masked embeddings; g_e = mask · g_x / keep; the oracle's _node_backward."""
    orc = _Oracle(prob)
    uniq, inv = np.unique(np.concatenate([q, db]), return_inverse=True)
    ent = [orc.entry(gi, c, seed) for c, gi in enumerate(uniq)]
    emb = np.stack([e[0] for e in ent])
    qp, dp = inv[:len(q)], inv[len(q):]
    y = labels.astype(np.float64)
    ystats = np.array([y.mean(), 0.5 * ((y - y.mean()) ** 2).sum()])
    _, loss, _, _, gq, gdb, head = _autograd_head(prob, emb[qp], emb[dp], labels, ystats, True)
    gx = np.zeros_like(emb)
    np.add.at(gx, qp, gq)
    np.add.at(gx, dp, gdb)
    G = {k: np.zeros_like(v) for k, v in orc.P.items()}
    for c, gi in enumerate(uniq):
        _, m, caches, shape = ent[c]
        O._node_backward(orc.spec, orc.P, G, orc.gs[gi], caches,
                         np.where(m, gx[c] / orc.keep, 0.0).reshape(shape))
    for name, g in head.items():
        G[(orc.hi, name)] = g
    return loss, O.flatten(orc.spec, G)


GRID_SHAPES = ('9x65', '7x7')


@pytest.mark.parametrize('shape', GRID_SHAPES)
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('stack', list(STACKS))
def test_grid_fwd_bwd_graph_dropout_matches_reference(gpu, stack, keep, shape):
    from graphembedding_amd.allpairs import AllPairsGrid, GraphSet
    from graphembedding_amd.packer import GraphStore
    prob, model, store, dev = _case(stack, keep, gpu)
    model.step_count = 0
    rng = np.random.default_rng(2)
    if shape == '9x65':     # graphs 0, 3, 10 and 64 in both roles; 70 distinct: 35 units
        q, db = np.array([3, 10, 64, 65, 66, 67, 68, 69, 0]), np.arange(65)
        labels = rng.uniform(0.05, 1.0, size=(9, 65)).astype(np.float32)
        seed = SEED
        model.grid_fwd_bwd(store, labels, q, db, dropout='graph', seed=seed).check()
        ref_prob = prob
    else:                   # the all-pairs grid of seven graphs: an odd tail
        import dataclasses
        ref_prob = dataclasses.replace(prob, graphs=prob.graphs[:7], mgs=prob.mgs[:7])
        q = db = np.arange(7)
        labels = rng.uniform(0.05, 1.0, size=(7, 7)).astype(np.float32)
        store7 = GraphStore(ref_prob.mgs, model.n_max, prob.d_in)
        gs = GraphSet(graphs=ref_prob.graphs, mgs=ref_prob.mgs, d_in=prob.d_in,
                      n_max=model.n_max, store=store7, ged=None)
        grid = AllPairsGrid(gs, labels, gpu, dropout='graph')
        seed = model._seed(None)                # the step's seed: the train steps' stream
        grid.fwd_bwd(model)
        gp = grid.problem(model)
        gp.check()
        assert gp.identity and gp.dropout == 'graph'
    g_gpu = model.grad.cpu().numpy().copy()
    l_gpu = float(model.loss_buf[0].item())
    l_ref, g_ref = _reference_step(ref_prob, q, db, labels, seed)
    print(stack, keep, shape, 'loss', l_gpu, 'reference', l_ref)
    assert abs(l_gpu - l_ref) <= TRAIN_TOL * max(1.0, abs(l_ref)), (l_gpu, l_ref)
    print(check_grad_per_var(g_gpu, g_ref, prob.layers, prob.d_in, TRAIN_TOL,
                             'graph dropout vs float64 reference'))
    # the masks matter: another seed's reference gradient is far outside the bar
    _, g_other = _reference_step(ref_prob, q, db, labels, seed + 1)
    assert np.abs(g_other - g_ref).max() > 10 * TRAIN_TOL * np.abs(g_ref).max()


# ---- 6. invalid entries ------------------------------------------------------------------
def test_embed_drop_invalid_entries(gpu):
    """An id outside the store and a node count above the Padding rows: the device status
    of sg_embed, zero rows, nothing in the gradient (the calls without them: the remaining
    entries under their own entry numbers)."""
    import torch
    from graphembedding_amd import _lib
    prob, model, store, dev = _case('default', 0.5, gpu)
    E = model.embed_dim
    adj, types, n = dev
    big = n.clone()
    big[21] = 11                                          # Padding(10) takes 10 rows (A9)
    good, st = _embed_drop(model, dev, [3, 0, 2, 1, 20, 21], SEED)
    assert st == 0
    out, st = _embed_drop(model, dev, [3, 10_000, 2, 1, 20, -1], SEED)
    assert st == _lib.SG_ERR_ARG
    assert not out[1].any() and not out[5].any()
    assert torch.equal(out[[0, 2, 3, 4]], good[[0, 2, 3, 4]])
    out, st = _embed_drop(model, (adj, types, big), [3, 0, 2, 1, 20, 21], SEED)
    assert st == _lib.SG_ERR_SHAPE and not out[5].any()
    assert torch.equal(out[:5], good[:5])
    out, st = _embed_drop(model, dev, [10_000, -5, 2], SEED)   # a whole unit, then an odd tail
    assert st == _lib.SG_ERR_ARG and not out[:2].any() and torch.equal(out[2], good[2])
    # the gradient: entries 1 (bad id) and 5 (bad node count) add nothing
    g_emb = np.random.default_rng(6).standard_normal((6, E)).astype(np.float32)
    got, st = _embed_drop_bwd(model, (adj, types, big), [3, 10_000, 2, 1, 20, 21], SEED, g_emb)
    assert st in (_lib.SG_ERR_ARG, _lib.SG_ERR_SHAPE)
    parts = [_embed_drop_bwd(model, dev, [3], SEED, g_emb[0:1], entry_offset=0),
             _embed_drop_bwd(model, dev, [2, 1], SEED, g_emb[2:4], entry_offset=2),
             _embed_drop_bwd(model, dev, [20], SEED, g_emb[4:5], entry_offset=4)]
    assert all(st == 0 for _, st in parts)
    head0 = _offsets(prob)[0][(len(prob.layers) - 1, 'weights_W')][0]
    want = got.copy()
    want[:head0] = sum(p[0][:head0].astype(np.float64) for p in parts)
    assert np.abs(want[:head0]).max() > 1e-3
    _node_blocks_close(prob, got, want)


# ---- 7. the Python surface ---------------------------------------------------------------
def test_grid_dropout_python_surface(gpu):
    from graphembedding_amd import _lib
    prob, _, store, dev = _case('default', 0.9, gpu)
    model = gpu_model(prob, gpu, learning_rate=0.0, weight_decay=0.0)
    assert model.flags.dropout == pytest.approx(0.1)
    q, db = np.arange(5), np.arange(3, 12)
    labels = np.random.default_rng(8).uniform(0.05, 1.0, size=(5, 9)).astype(np.float32)
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.grid_problem(store, labels, q, db)                  # dropout=None: today's refusal
    with pytest.raises(_lib.SiameseHipError, match='dropout'):
        model.grid_fwd_bwd(store, labels, q, db)
    for bad in ('pair', 'Graph', True, 0.1):
        with pytest.raises(_lib.SiameseHipError, match="None or 'graph'"):
            model.grid_problem(store, labels, q, db, dropout=bad)
        with pytest.raises(_lib.SiameseHipError, match="None or 'graph'"):
            model.grid_fwd_bwd(store, labels, q, db, dropout=bad)
    gp = model.grid_problem(store, labels, q, db, dropout='graph')
    assert gp.dropout == 'graph' and model.step_count == 0
    # Adam with a zero learning rate moves nothing: two steps differ by their masks alone
    before = model.params.clone()
    l0 = model.grid_train_step(gp)
    l1 = model.grid_train_step(gp)
    gp.check()
    assert model.step_count == 2
    assert model.torch.equal(model.params, before)
    assert l0 != l1, (l0, l1)
    # the same step again: the same loss
    model.step_count = 0
    assert model.grid_train_step(gp) == l0
    # dropout='graph' at flags.dropout = 0 is the existing path
    plain = gpu_model(prob, gpu, dropout=0.0)
    plain.grid_fwd_bwd(store, labels, q, db)
    g_none, l_none = plain.grad.cpu().numpy().copy(), float(plain.loss_buf[0].item())
    plain.grid_fwd_bwd(store, labels, q, db, dropout='graph')
    assert float(plain.loss_buf[0].item()) == l_none
    print(check_grad_per_var(plain.grad.cpu().numpy(), g_none, prob.layers, prob.d_in, TRAIN_TOL,
                             "dropout='graph' vs None at dropout 0"))
