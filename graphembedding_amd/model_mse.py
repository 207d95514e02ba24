"""SiameseGCNTNMSE — host mirror of model/Siamese/model_mse.py:9-168 +
models.py:6-131 on top of the HIP C-ABI.

What was `sess.run` in the reference is now a sequence of stream-ordered
C-ABI calls on torch's current stream:
  train  (train.py:85)  sg_fwd_bwd → [all-reduce] → sg_adam_tf
  val    (train.py:86)  sg_fwd_bwd (loss only)
  test   (train.py:87)  sg_forward → pre-activation s (pred_sim_without_act)
Parameters are one flat fp32 device vector in the reference's variable order.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .config import FLAGS
from .layers_factory import create_activation, create_layers, padding_dims
from .packer import GraphStore, record_words
from .similarity import create_sim_kernel


def param_shapes(layers: List[dict], d_in: int) -> List[Tuple[int, str, Tuple[int, ...]]]:
    """(layer index, variable name, shape) in variable creation order
    (layers.py:68-73, 151-152, 174-178, 268-277)."""
    out = []
    for li, L in enumerate(layers):
        k = L['kind']
        if k == 'GraphConvolution':
            din = L.get('input_dim') or d_in
            out.append((li, 'weights_0', (din, L['output_dim'])))
            if L['bias']:
                out.append((li, 'bias', (L['output_dim'],)))
        elif k == 'Dense':
            out.append((li, 'weights', (L['input_dim'], L['output_dim'])))
            if L['bias']:
                out.append((li, 'bias', (L['output_dim'],)))
        elif k == 'Attention':
            out.append((li, 'weights', (L['input_dim'], L['input_dim'])))
        elif k == 'NTN':
            D, K = L['input_dim'], L['feature_map_dim']
            out += [(li, 'weights_W', (D, D, K)), (li, 'weights_V', (K, 2 * D)),
                    (li, 'weights_U', (K, 1))]
            if L['bias']:
                out.append((li, 'bias', (K,)))
    return out


def glorot_flat(layers: List[dict], d_in: int, seed: int = 0) -> np.ndarray:
    """inits.py:11-21 (uniform ±√(6/(s0+s1)); zeros for biases), numpy-seeded."""
    rng = np.random.default_rng(seed)
    parts = []
    for li, name, shape in param_shapes(layers, d_in):
        if name == 'bias':
            parts.append(np.zeros(shape))
        else:
            r = math.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-r, r, size=shape))
    return np.concatenate([p.ravel() for p in parts]).astype(np.float32)


def splitmix64(x: int) -> int:
    """Steele et al.'s splitmix64 finaliser (a bijection of 64-bit integers)."""
    m = 0xFFFFFFFFFFFFFFFF
    x = (int(x) + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _distinct_index(g1s: Sequence, g2s: Sequence):
    """(distinct graphs in order of first appearance, int32 [n, 2] index of every pair's
    two graphs among them); graphs are told apart by identity."""
    uniq, index = [], {}
    idx = np.zeros((len(g1s), 2), np.int32)
    for k, (a, b) in enumerate(zip(g1s, g2s)):
        for c, g in enumerate((a, b)):
            if id(g) not in index:
                index[id(g)] = len(uniq)
                uniq.append(g)
            idx[k, c] = index[id(g)]
    return uniq, idx


def _label_stats(torch, lab, count):
    """float32 [2] {ȳ, ½Σ(y−ȳ)²} of the label tensor, computed in float64 on its device
    (ȳ = 0 for an empty set, count = 0)."""
    y64 = lab.double()
    ybar = y64.mean() if count else torch.zeros((), dtype=torch.float64, device=lab.device)
    return torch.stack([ybar, 0.5 * ((y64 - ybar) ** 2).sum()]).float()


@dataclass
class Batch:
    """A packed batch resident on the device (what get_feed_dict returns)."""
    records: object                 # torch.int32 [n * record_words]
    n_pairs: int
    labels: object                  # torch.float32 [n] (per input pair, for aligned loss)
    y_stats: object                 # torch.float32 [2] {ȳ, ½Σ(y-ȳ)²} of the label set
    pair_offset: int = 0            # global index of record 0 (dropout RNG / sharding)
    batch_total: int = 0            # global batch size B
    gid_pairs: Optional[np.ndarray] = None
    order: object = None            # torch.int32 [n] processing order (balance()) or None
    cls: object = None              # torch.int32 [5] class table of the order (fused path)
    # graph-store path (kernel path 3, config C5): pair ids into a CSR store instead of records
    csr: object = None              # web.CsrStore
    pairs: object = None            # torch.int32 [n, 2] store graph ids
    chunk: int = 0                  # pairs per internal chunk (workspace size)
    # store-sourced pairs (library 1.6, kernel path 2): the fused kernel gathers each pair
    # from a dense GraphStore instead of a packed record (records is None)
    src: object = None              # _lib.SgPairSource
    src_keep: tuple = ()            # the device tensors src points into (kept alive)


@dataclass
class GridProblem:
    """An m x n block of pairs for embed-once training (SiameseGCNTNMSE.grid_problem):
    device tensors only, so a step runs without host work."""
    store_dev: tuple                # (adj, types, n) of the GraphStore
    m: int
    n: int
    labels: object                  # torch.float32 [m][n]
    y_stats: object                 # torch.float32 [2] {ȳ, ½Σ(y-ȳ)²}
    uniq: object                    # torch.int32 [U] distinct store graphs, ascending
    q_pos: object                   # torch.int64 [m] position of query i in uniq
    db_pos: object                  # torch.int64 [n] position of database j in uniq
    identity: bool                  # queries = database = uniq (the all-pairs grid)
    emb: object                     # [U][E] embeddings
    g_emb: object                   # [U][E] their gradients (query role + database role)
    g_q: object                     # [m][E]
    g_db: object                    # [n][E]
    status: object                  # torch.int32 [1] device status of sg_embed / sg_embed_bwd
    ws_grid: object
    ws_embed: object
    dropout: Optional[str] = None   # None: dropout 0 only; 'graph': one mask set per graph
    # graph-store (Web) problems (web_grid_problem): store_dev is (CsrStore, its device
    # struct), the embedding buffers are [*][ld] (ld = D rounded up to 128)
    ws_fwd: object = None           # workspace of sg_web_embed / sg_web_embed_drop

    def check(self):
        """Raise if a kernel reported a bad graph id or node count (synchronises)."""
        _lib.check(int(self.status.item()), 'embed-once training (device status)')


class _Family(object):
    """How a model's family talks to the library in the embed-once calls: the ctypes wrappers
    it uses (a name that is None: the family has no such call) and what differs in their
    argument lists.
      strided  the grid calls take embeddings with a row stride, else contiguous [*, E] copies
      params   the grid calls take the parameter vector (the Dot head has no variables)
      web      the store is a CsrStore's struct, the embedding buffers are [*][ld] rows, the
               embed calls take a workspace and the backward calls the gradients' row stride"""

    def __init__(self, strided, params, web, **calls):
        self.strided, self.params, self.web = strided, params, web
        self.__dict__.update(calls)


_NODE_STACK = dict(embed=_lib.embed, embed_drop=_lib.embed_drop, embed_bwd=_lib.embed_bwd,
                   embed_drop_bwd=_lib.embed_drop_bwd, embed_ws=None, embed_drop_ws=None,
                   embed_bwd_ws=_lib.embed_bwd_workspace_bytes,
                   embed_drop_bwd_ws=_lib.embed_drop_bwd_workspace_bytes)
_FAMILIES = {
    'ntn': _Family(strided=False, params=True, web=False, grid=_lib.score_grid,
                   grid_ws=_lib.score_grid_workspace_bytes, search=_lib.search_topk,
                   search_ws=_lib.search_workspace_bytes,
                   grid_fwd_bwd=_lib.score_grid_fwd_bwd,
                   grid_bwd_ws=_lib.score_grid_bwd_workspace_bytes, **_NODE_STACK),
    'dot': _Family(strided=True, params=False, web=False, grid=_lib.dot_score_grid, grid_ws=None,
                   search=_lib.dot_search_topk, search_ws=_lib.dot_search_workspace_bytes,
                   grid_fwd_bwd=_lib.dot_score_grid_fwd_bwd,
                   grid_bwd_ws=_lib.dot_score_grid_bwd_workspace_bytes, **_NODE_STACK),
    'web': _Family(strided=True, params=True, web=True, grid=_lib.web_score_grid,
                   grid_ws=_lib.web_score_grid_workspace_bytes, search=_lib.web_search_topk,
                   search_ws=_lib.web_search_workspace_bytes,
                   grid_fwd_bwd=_lib.web_score_grid_fwd_bwd,
                   grid_bwd_ws=_lib.web_score_grid_bwd_workspace_bytes,
                   embed=_lib.web_embed, embed_drop=_lib.web_embed_drop,
                   embed_bwd=_lib.web_embed_bwd, embed_drop_bwd=_lib.web_embed_drop_bwd,
                   embed_ws=_lib.web_embed_workspace_bytes,
                   embed_drop_ws=_lib.web_embed_drop_workspace_bytes,
                   embed_bwd_ws=_lib.web_embed_bwd_workspace_bytes,
                   embed_drop_bwd_ws=_lib.web_embed_drop_bwd_workspace_bytes),
}


class SiameseGCNTNMSE(object):
    def __init__(self, input_dim, flags=None, device='cuda', n_max=None, params=None):
        f = flags or FLAGS
        assert f.loss_func == 'mse'
        self.flags = f
        self.input_dim = int(input_dim)
        self.device = device
        self.layers = create_layers(f, self.input_dim)
        pd = padding_dims(self.layers)
        self.n_max = int(n_max or f.n_max or pd or 10)
        # the reference's tf.pad fails for N > max_in_dims (layers.py:226, quirk A9); the
        # kernels would drop the extra nodes instead, so every store is checked on entry
        # (check_node_counts) even when the record capacity n_max exceeds the Padding dim
        self.max_nodes = pd
        self.sim_kernel = create_sim_kernel(f.sim_kernel, f.yeta)
        self.final_act_np = create_activation(f.final_act, self.sim_kernel)
        self.record_dtype = getattr(f, 'record_dtype', 'f32') or 'f32'
        def make(cap):
            return _lib.make_model(self.layers, self.input_dim, cap, 1.0 - f.dropout,
                                   f.final_act, f.sim_kernel, f.yeta, f.loss_mode, f.ntn_mode,
                                   self.record_dtype)
        self.sg = make(self.n_max)
        self.n_params, self.kernel_path = _lib.validate(self.sg)
        # Record node capacity: any capacity >= the largest graph is valid, and the
        # fused kernels want a specific one (the Padding dim <= 12, or 32 for
        # Padding dims in (12, 31]: config C4), so take it when the stack qualifies.
        if self.kernel_path == 0 and pd is not None and self.n_max <= pd:
            for cap in (pd, 32):
                if cap <= self.n_max:
                    continue
                sg2 = make(cap)
                n2, path2 = _lib.validate(sg2)
                if path2:
                    self.sg, self.n_max, self.n_params, self.kernel_path = sg2, cap, n2, path2
                    break
        # the family of the embed-once calls (_Family)
        self._family = _FAMILIES['web' if self.is_web else 'dot' if self.is_dot else 'ntn']
        import torch
        self.torch = torch
        init = glorot_flat(self.layers, self.input_dim, f.param_seed) if params is None else \
            np.asarray(params, np.float32)
        assert init.shape[0] == self.n_params, (init.shape, self.n_params)
        self.params = torch.from_numpy(init.copy()).to(device)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.beta1, self.beta2, self.eps = 0.9, 0.999, 1e-8
        self.beta_powers = torch.tensor([self.beta1, self.beta2], dtype=torch.float32, device=device)
        # grad and loss_mse share one flat buffer: the data-parallel all-reduce
        # (shard.make_allreduce_hook) is then a single in-place collective
        n = self.params.numel()
        self.grad_loss = torch.zeros(n + 2, dtype=torch.float32, device=device)
        self.grad = self.grad_loss[:n]
        self.loss_buf = self.grad_loss[n:]
        self.reg_buf = torch.zeros(1, dtype=torch.float32, device=device)
        self._ws = None
        self._ws_pairs = -1
        self.seed = int(f.seed)
        self.step_count = 0
        self.grad_hook = None   # e.g. the data-parallel all-reduce (shard.py)
        self._adam_ws = None
        if self.n_params > 65536:   # multi-block Adam (config C5: D²K NTN weights)
            self._adam_ws = torch.empty(_lib.adam_workspace_bytes(self.n_params) // 8 + 1,
                                        dtype=torch.float64, device=device)

    @property
    def is_web(self) -> bool:
        """Graph-store path (sg_web_*, config C5): Padding/NTN width in [32, 512]."""
        return self.kernel_path == _lib.PATH_WEB

    def check_node_counts(self, n_nodes, what='graph store'):
        """Raise like the reference's tf.pad (layers.py:226, quirk A9) when a graph has
        more nodes than the Padding layer's max_in_dims."""
        n = np.asarray(n_nodes).reshape(-1)
        if self.max_nodes is not None and n.size and int(n.max()) > self.max_nodes:
            k = int(np.argmax(n))
            raise _lib.SiameseHipError(
                '{}: graph {} has {} nodes > Padding max_in_dims {} (layers.py:226)'.format(
                    what, k, int(n[k]), self.max_nodes))

    def _check_store_capacity(self, store):
        """The kernels index a dense store by the model's capacity: its slots must be n_max."""
        if store.n_max != self.n_max:
            raise _lib.SiameseHipError('store n_max {} != model n_max {}'.format(store.n_max,
                                                                                 self.n_max))

    # ---- reference API ------------------------------------------------------
    def apply_final_act_np(self, score):
        return self.final_act_np(score)

    def pred_sim_without_act(self, batch: Batch, seed: Optional[int] = None):
        """Pre-activation scores of the batch (train.py:87 'test')."""
        torch = self.torch
        s = torch.empty(batch.n_pairs, dtype=torch.float32, device=self.device)
        if batch.csr is not None:
            _lib.web_forward(self.sg, batch.csr.to_device(self.device), batch.pairs, batch.n_pairs,
                             batch.pair_offset, self.params, self._seed(seed), s,
                             self.web_workspace(batch.chunk, batch.n_pairs), batch.chunk)
            return s
        if batch.src is not None:
            _lib.forward_src(self.sg, batch.src, batch.n_pairs, batch.pair_offset, self.params,
                             self._seed(seed), s, order=batch.order)
            return s
        _lib.forward(self.sg, batch.records, batch.n_pairs, batch.pair_offset, self.params,
                     self._seed(seed), s, order=batch.order, class_start=batch.cls)
        return s

    def get_feed_dict(self, data, dist_calculator, tvt, test_id=None, train_id=None):
        """model_mse.py:52-94, same sampler-call pattern (quirk A3 in 'compat')."""
        B = self.flags.batch_size
        if tvt in ('train', 'val'):
            assert test_id is None and train_id is None
            pairs = [data.get_graph_pair(tvt) for _ in range(B)]
        else:
            assert tvt == 'test'
            pairs = [(data.test_data.get_graph(test_id), data.get_orig_train_graph(train_id))]
        dists = norm_dists = None
        if tvt in ('train', 'val'):
            if self.flags.label_stream == 'compat':
                # the label block sits inside the per-pair loop: B redraws of B pairs
                for _ in range(len(pairs)):
                    dists, norm_dists = np.zeros(B), np.zeros(B)
                    for i in range(B):
                        g1, g2 = data.get_graph_pair(tvt)
                        d, nd = data.get_dist(g1.get_nxgraph(), g2.get_nxgraph(), dist_calculator)
                        dists[i], norm_dists[i] = d, nd
            else:
                dists, norm_dists = np.zeros(B), np.zeros(B)
                for i, (g1, g2) in enumerate(pairs):
                    d, nd = data.get_dist(g1.get_nxgraph(), g2.get_nxgraph(), dist_calculator)
                    dists[i], norm_dists[i] = d, nd
        labels = None
        if dists is not None:
            d = norm_dists if self.flags.dist_norm else dists
            labels = self.sim_kernel.dist_to_sim_np(np.asarray(d, np.float32).astype(np.float64))
        return self.make_batch([p[0] for p in pairs], [p[1] for p in pairs], labels)

    def make_batch(self, g1s: Sequence, g2s: Sequence, labels=None, pair_offset=0,
                   batch_total=None) -> Batch:
        """Pack ModelGraph pairs on the host and move them to the device."""
        torch = self.torch
        if self.is_web:
            return self.make_web_batch(g1s, g2s, labels, pair_offset, batch_total)
        uniq, idx = _distinct_index(g1s, g2s)
        store = GraphStore(uniq, self.n_max, self.input_dim)
        self.check_node_counts(store.n, 'make_batch')
        lab = np.zeros(len(g1s), np.float32) if labels is None else np.asarray(labels, np.float32)
        words = store.pack_host(idx, lab, dtype=self.record_dtype)
        recs = torch.from_numpy(words.view(np.int32).reshape(-1)).to(self.device)
        gids = np.array([[a.nxgraph.graph.get('gid', -1), b.nxgraph.graph.get('gid', -1)]
                         for a, b in zip(g1s, g2s)])
        return self.batch_from_records(recs, len(g1s), lab, pair_offset, batch_total, gids)

    def make_web_batch(self, g1s: Sequence, g2s: Sequence, labels=None, pair_offset=0,
                       batch_total=None, chunk=None) -> Batch:
        """ModelGraph pairs → a CSR store of the distinct graphs + pair ids (path 3)."""
        from .web import CsrStore
        torch = self.torch
        uniq, idx = _distinct_index(g1s, g2s)
        store = CsrStore(uniq, self.input_dim, self.n_max)
        lab = np.zeros(len(g1s), np.float32) if labels is None else np.asarray(labels, np.float32)
        gids = np.array([[a.nxgraph.graph.get('gid', -1), b.nxgraph.graph.get('gid', -1)]
                         for a, b in zip(g1s, g2s)])
        b = self.web_batch(store, torch.from_numpy(idx).to(self.device), lab, pair_offset,
                           batch_total, chunk=chunk)
        b.gid_pairs = gids
        return b

    def web_batch(self, store, pairs, labels, pair_offset=0, batch_total=None, y_stats=None,
                  chunk=None) -> Batch:
        n = int(pairs.shape[0])
        self.check_node_counts(store.n, 'web_batch')
        b = self.batch_from_records(None, n, labels, pair_offset, batch_total, y_stats=y_stats)
        b.csr, b.pairs = store, pairs
        b.chunk = int(chunk or min(max(n, 1), 32768))
        return b

    def web_workspace(self, chunk, n_pairs=-1):
        """Graph-store workspace for calls of up to n_pairs pairs in chunks of `chunk`
        (n_pairs <= chunk: one pipeline slot, about half the bytes; -1: any n_pairs).  A
        cached workspace is reused when it is at least as large as the call needs."""
        torch = self.torch
        one = 0 <= int(n_pairs) <= int(chunk)
        key = ('web', int(chunk), one)
        have = getattr(self, '_web_ws_key', None)
        if have is not None and have[:2] == key[:2] and (not have[2] or one):
            return self._web_ws
        nbytes = _lib.web_workspace_bytes(self.sg, int(chunk), 0 if one else -1)
        self._web_ws = None
        self._web_ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
        self._web_ws_key = key
        return self._web_ws

    def batch_from_records(self, recs, n_pairs, labels, pair_offset=0, batch_total=None,
                           gid_pairs=None, y_stats=None) -> Batch:
        torch = self.torch
        if recs is not None:   # the kernels read n_pairs whole records
            need = int(n_pairs) * record_words(self.n_max, self.record_dtype)
            if recs.numel() * recs.element_size() < 4 * need:
                raise _lib.SiameseHipError('records hold fewer than n_pairs = {} records of '
                                           '{} B'.format(int(n_pairs), 4 * need // max(1, int(n_pairs))))
        lab = torch.as_tensor(np.asarray(labels, np.float32) if not torch.is_tensor(labels)
                              else labels, dtype=torch.float32, device=self.device)
        if y_stats is None:
            y_stats = _label_stats(torch, lab, n_pairs)
        return Batch(records=recs, n_pairs=int(n_pairs), labels=lab, y_stats=y_stats,
                     pair_offset=int(pair_offset),
                     batch_total=int(batch_total if batch_total is not None else n_pairs),
                     gid_pairs=gid_pairs)

    def batch_from_store(self, store, n_pairs, labels, pair_idx=None, grid_base=0,
                         pair_offset=0, batch_total=None, y_stats=None, status=None) -> Batch:
        """A batch whose pairs the fused kernel gathers from the dense store itself
        (sg_*_src, library 1.6; kernel paths 1 and 2 with f32 Â): store = packer.GraphStore,
        pair_idx int32 [n, 2] device tensor or None for the all-pairs grid (pair i =
        divmod(grid_base + i, G)), labels float32 [n] device tensor.  Same results as
        packing the pairs into records (sg_pack_pairs) and stepping those."""
        if self.kernel_path not in (1, 2) or self.record_dtype != 'f32':
            raise _lib.SiameseHipError('store-sourced batches need a fused kernel path with '
                                       'f32 records (kernel path {})'.format(self.kernel_path))
        self._check_store_capacity(store)
        torch = self.torch
        n_pairs = int(n_pairs)
        self.check_node_counts(store.n, 'batch_from_store')
        # the kernel reads pair_idx[0 .. 2n) and labels[0 .. n): check before it does
        if pair_idx is not None:
            if (not torch.is_tensor(pair_idx) or pair_idx.dtype != torch.int32 or
                    not pair_idx.is_contiguous() or pair_idx.numel() < 2 * n_pairs):
                raise _lib.SiameseHipError('pair_idx must be a contiguous int32 [n, 2] tensor')
        elif int(grid_base) < 0:
            raise _lib.SiameseHipError('grid_base must be >= 0')
        if torch.is_tensor(labels) and labels.numel() < n_pairs:
            raise _lib.SiameseHipError('labels has fewer than n_pairs entries')
        dev = store.to_device(self.device)
        b = self.batch_from_records(None, n_pairs, labels, pair_offset=pair_offset,
                                    batch_total=batch_total, y_stats=y_stats)
        b.src = _lib.pair_source(dev, store.n_max, pair_idx=pair_idx, grid_base=grid_base,
                                 labels=b.labels, status=status)
        b.src_keep = (dev, pair_idx, b.labels, status)
        return b

    # ---- steps ----------------------------------------------------------------
    def _seed(self, seed):
        return (self.seed * 1000003 + self.step_count) if seed is None else int(seed)

    def workspace(self, n_pairs):
        torch = self.torch
        if self._ws is None or n_pairs > self._ws_pairs:
            nbytes = _lib.workspace_bytes(self.sg, max(int(n_pairs), 1))
            self._ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=self.device)
            self._ws_pairs = int(n_pairs)
        return self._ws

    def fwd_bwd(self, batch: Batch, seed=None, s_out=None, add_label_term=True):
        """Forward + loss + backward; leaves Σ∂loss_mse/∂θ in self.grad and the
        shard's loss_mse in self.loss_buf[0]."""
        if batch.csr is not None:
            _lib.web_fwd_bwd(self.sg, batch.csr.to_device(self.device), batch.pairs, batch.labels,
                             batch.n_pairs, batch.pair_offset, batch.batch_total, self.params,
                             self._seed(seed), batch.y_stats, 1 if add_label_term else 0, s_out,
                             self.grad, self.loss_buf,
                             self.web_workspace(batch.chunk, batch.n_pairs), batch.chunk)
            return
        if batch.src is not None:
            _lib.fwd_bwd_src(self.sg, batch.src, batch.n_pairs, batch.pair_offset,
                             batch.batch_total, self.params, self._seed(seed), batch.y_stats,
                             1 if add_label_term else 0, s_out, self.grad, self.loss_buf,
                             self.workspace(batch.n_pairs), order=batch.order)
            return
        _lib.fwd_bwd(self.sg, batch.records, batch.n_pairs, batch.pair_offset,
                     batch.batch_total, self.params, self._seed(seed), batch.y_stats,
                     1 if add_label_term else 0, s_out, self.grad, self.loss_buf,
                     self.workspace(batch.n_pairs), order=batch.order, class_start=batch.cls)

    # SG_CLASS_SCHEDULE=0 keeps the mixed (snake) schedule on the fused path
    CLASS_SCHEDULE = True

    def balance(self, batch: Batch, classes: Optional[bool] = None) -> Batch:
        """Attach the class-sorted processing order of the batch's records
        (sg_pair_order): every wavefront then gets the same mix of cheap and
        expensive pairs.  On the fused path (kernel path 1) the order comes with its
        class table (sg_pair_order_cls) and every wavefront runs the pairs of one class
        (class-exclusive schedule).  Scores are unchanged; the gradient differs only by
        summation order.  Worth it for batches that are stepped repeatedly (all-pairs
        epochs), not for the reference's B = 5 feeds."""
        import os
        torch = self.torch
        if batch.n_pairs == 0 or batch.csr is not None:
            return batch
        if classes is None:
            classes = self.CLASS_SCHEDULE and os.environ.get('SG_CLASS_SCHEDULE', '1') != '0'
        ws = torch.empty(_lib.pair_order_workspace_bytes(self.sg, batch.n_pairs) // 4 + 1,
                         dtype=torch.int32, device=self.device)
        order = torch.empty(batch.n_pairs, dtype=torch.int32, device=self.device)
        batch.cls = None
        if batch.src is not None:
            _lib.pair_order_src(self.sg, batch.src, batch.n_pairs, order, ws)
        elif classes and self.kernel_path == 1:
            cls = torch.empty(_lib.FAST_CLASSES_P1, dtype=torch.int32, device=self.device)
            _lib.pair_order_cls(self.sg, batch.records, batch.n_pairs, order, cls, ws)
            batch.cls = cls
        else:
            _lib.pair_order(self.sg, batch.records, batch.n_pairs, order, ws)
        batch.order = order
        return batch

    def apply_adam(self):
        f = self.flags
        if self._adam_ws is not None:
            _lib.adam_tf_ex(self.params, self.adam_m, self.adam_v, self.grad, f.learning_rate,
                            self.beta1, self.beta2, self.eps, f.weight_decay, self.beta_powers,
                            self.reg_buf, self._adam_ws)
            return
        _lib.adam_tf(self.params, self.adam_m, self.adam_v, self.grad, f.learning_rate,
                     self.beta1, self.beta2, self.eps, f.weight_decay, self.beta_powers,
                     self.reg_buf)

    def fwd_bwd_adam(self, batch: Batch, seed=None, s_out=None, add_label_term=True):
        """fwd_bwd + apply_adam as one library call (sg_train_step: on the fused path the
        gradient reduction applies Adam in the same launch).  Same results as the two calls
        (θ, m, v, grad, loss bitwise; reg_buf summed in another order).  Record batches
        only; other batches take the two calls."""
        if batch.csr is not None or batch.src is not None or self._adam_ws is not None:
            self.fwd_bwd(batch, seed, s_out, add_label_term)
            self.apply_adam()
            return
        f = self.flags
        _lib.train_step(self.sg, batch.records, batch.n_pairs, batch.pair_offset,
                        batch.batch_total, self.params, self._seed(seed), batch.y_stats,
                        1 if add_label_term else 0, s_out, self.grad, self.loss_buf,
                        self.workspace(batch.n_pairs), self.adam_m, self.adam_v,
                        f.learning_rate, self.beta1, self.beta2, self.eps, f.weight_decay,
                        self.beta_powers, self.reg_buf, order=batch.order,
                        class_start=batch.cls)

    def train_step(self, batch: Batch, seed=None, sync=True):
        """sess.run([opt_op, loss]) (train.py:85,92): returns the loss evaluated
        at the pre-update parameters (incl. weight decay, models.py:67-88)."""
        if self.grad_hook is None:
            self.fwd_bwd_adam(batch, seed)
        else:
            self.fwd_bwd(batch, seed)
            self.grad_hook(self)
            self.apply_adam()
        self.step_count += 1
        if not sync:
            return None
        return float(self.loss_buf[0].item() + self.reg_buf[0].item())

    def capture_train_steps(self, feed, n_steps: int = 1):
        """A hipGraph of n_steps reference train steps (train.py:8-44: get_feed_dict
        then sess.run([opt_op, loss]) with B = 5 pairs): DeviceFeed.next_batch →
        sg_fwd_bwd_dseed → ApplyAdam → seed + 1, all stream-ordered with no host sync.
        The dropout seed lives on the device, so every replay draws the masks an eager
        step with the same step_count would.  Returns a GraphSteps whose replay() runs
        the captured steps; fused path (default / Average stack) only."""
        return GraphSteps(self, feed, n_steps)

    # validation draws its dropout masks from a stream of its own: the reference's val
    # sess.run (train.py:19-21) samples independently of the train steps
    VAL_SEED_STREAM = 0x5641_4C5F_5354_524D   # 'VAL_STRM'

    def val_seed(self, seed=None):
        """An explicit seed is used as given; the default is the step's seed tagged with
        the validation stream and put through splitmix64, so both 32-bit halves (and the
        kernels' 32-bit key lo*C ^ hi) change in every bit position, not by one fixed
        XOR of the train key (which would make a val pair's masks another pair's train
        masks)."""
        if seed is not None:
            return int(seed)
        return splitmix64(self._seed(None) ^ self.VAL_SEED_STREAM)

    def val_loss(self, batch: Batch, seed=None):
        """sess.run([merged, loss]) on valid_data (train.py:19-21): the loss at the current
        parameters, with independent dropout masks (val_seed); self.grad / loss_buf keep
        the last training step's values."""
        saved = self.grad_loss.clone()
        self.fwd_bwd(batch, self.val_seed(seed))
        loss = float(self.loss_buf[0].item())
        self.grad_loss.copy_(saved)
        reg = self.flags.weight_decay * 0.5 * float((self.params.double() ** 2).sum().item())
        return loss + reg

    def test_scores(self, batch: Batch, seed=None):
        return self.pred_sim_without_act(batch, seed).cpu().numpy().astype(np.float64)

    # ---- embed-once retrieval, search and training ------------------------------------------
    # A model belongs to one family (_Family above): 'ntn' (include/siamese_embed.h,
    # siamese_search.h, siamese_embed_train.h, siamese_embed_drop.h), 'dot' (the node-stack
    # calls of 'ntn', the grid calls of include/siamese_dot_embed.h) or 'web', graph-store
    # models (include/siamese_web_*.h).  _embed, _score_grid, _search, _grid_problem,
    # _grid_fwd_bwd and _grid_train_step are each written once on the family; the public
    # methods below them apply their refusal and name themselves in the messages.
    def _no_web(self, what):
        if self.is_web:
            raise _lib.SiameseHipError('{}: graph-store (Web) models have no embedding '
                                       'kernels here; use web_embed / web_score_grid / '
                                       'web_search / topk'.format(what))

    def _only_web(self, what):
        if not self.is_web:
            raise _lib.SiameseHipError('{}: the model is not on the graph-store (Web) path; '
                                       'use embed / score_grid'.format(what))

    @property
    def is_dot(self) -> bool:
        """The pair head is Dot (layers.py:230-252): the grid calls of
        include/siamese_dot_embed.h serve it, the NTN grid calls every other model."""
        return self.layers[-1]['kind'] == 'Dot'

    @property
    def embed_dim(self) -> int:
        """Width of one graph embedding: the pair head's per-graph input."""
        self._no_web('embed_dim')
        return _lib.embed_dim(self.sg)

    @property
    def web_embed_dim(self) -> int:
        """Width D of one graph embedding of a graph-store model: the Padding / NTN width."""
        self._only_web('web_embed_dim')
        return _lib.web_embed_dim(self.sg)

    def _embed_dims(self):
        """(width, row stride) of the embedding buffers: [*][E], or for graph-store models the
        [*][ld] rows of sg_web_embed (ld = D rounded up to 128)."""
        if self._family.web:
            return _lib.web_embed_dim(self.sg), _lib.web_embed_ld(self.sg)
        return 2 * (_lib.embed_dim(self.sg),)

    def _f32(self, shape, new=None):
        return (new or self.torch.empty)(shape, dtype=self.torch.float32, device=self.device)

    def _new_ws(self, nbytes):
        return self._f32(nbytes // 4 + 1)

    def _rows(self, e, d, what):
        """(tensor, row stride) of embeddings [*, d] as the strided grid calls take them: a
        tensor with unit inner stride and a row stride >= d is passed on as it is (the
        web_embed view with its stride of 128 or more), anything else is copied."""
        torch = self.torch
        e = torch.as_tensor(e, dtype=torch.float32, device=self.device)
        if e.dim() != 2 or e.shape[1] != d:
            raise _lib.SiameseHipError('{}: embeddings must be [*, {}]'.format(what, d))
        if e.stride(1) != 1 or (e.shape[0] > 1 and e.stride(0) < d):
            e = e.contiguous()
        return e, (int(e.stride(0)) if e.shape[0] > 1 else max(d, int(e.stride(0))))

    def _grid_operands(self, emb_q, emb_db, what):
        """(what every grid call starts with, m, n): the embeddings, with their row strides or
        as contiguous [*, E] copies, the two counts, and the parameters if the head has any."""
        fam, d = self._family, self._embed_dims()[0]
        (q, ld_q), (db, ld_db) = (self._rows(e, d, what) for e in (emb_q, emb_db))
        m, n = int(q.shape[0]), int(db.shape[0])
        ops = [q, ld_q, db, ld_db] if fam.strided else [q.contiguous(), db.contiguous()]
        return ops + [m, n] + ([self.params] if fam.params else []), m, n

    def _node_args(self, store_dev, idx, count, seed):
        """What every node-stack call starts with; seed: None, or the step's seed of graph-keyed
        dropout (entry c is side c & 1 of unit c >> 1: entry_offset 0)."""
        store = [store_dev] if self._family.web else [store_dev, self.n_max]
        return store + [idx, count] + ([self.params] if seed is None else [0, self.params, seed])

    def _embed_call(self, store_dev, idx, count, seed, out, ws, status):
        """sg_embed, or with a seed sg_embed_drop (sg_web_*: with their workspace), under the
        model's own struct."""
        fam = self._family
        (fam.embed if seed is None else fam.embed_drop)(
            self.sg, *self._node_args(store_dev, idx, count, seed), out,
            *([ws] if fam.web else []), status)

    def _embed(self, what, store, graph_idx):
        torch, fam = self.torch, self._family
        if not fam.web:
            self._check_store_capacity(store)
        self.check_node_counts(store.n, what)
        idx = None
        count = len(store)
        if graph_idx is not None:
            idx = torch.as_tensor(graph_idx, dtype=torch.int32, device=self.device).reshape(-1)
            idx = idx.contiguous()
            count = int(idx.numel())
        d, ld = self._embed_dims()
        out = self._f32((count, ld))
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = self._new_ws(fam.embed_ws(self.sg, count)) if fam.web else None
        self._embed_call(store.to_device(self.device), idx, count, None, out, ws, status)
        _lib.check(int(status.item()), 'sg_{} (device status)'.format(what))
        return out if ld == d else out[:, :d]

    def _score_grid(self, what, emb_q, emb_db, final):
        fam = self._family
        ops, m, n = self._grid_operands(emb_q, emb_db, what)
        ws = [self._new_ws(fam.grid_ws(self.sg, m))] if fam.grid_ws else []   # Dot: no workspace
        out = self._f32((m, n))
        fam.grid(self.sg, *ops, final, out, n, *ws)
        return out

    def _search(self, what, emb_q, emb_db, k, largest, final, seg_cols):
        torch, fam = self.torch, self._family
        ops, m, n = self._grid_operands(emb_q, emb_db, what)
        nbytes = fam.search_ws(self.sg, m, n, k, seg_cols)
        ws = getattr(self, '_search_ws', None)      # the last workspace, kept while it fits
        if ws is None or ws.numel() * 4 < nbytes or ws.device != ops[0].device:
            ws = self._new_ws(nbytes)
            self._search_ws = ws
        idx = torch.empty((m, int(k)), dtype=torch.int32, device=self.device)
        val = self._f32((m, int(k)))
        fam.search(self.sg, *ops, final, k, largest, seg_cols, idx, val, ws)
        return idx, val

    def embed(self, store: GraphStore, graph_idx=None):
        """Graph-level embeddings [count][embed_dim] (torch, on the device) of the graphs
        graph_idx (store ids, repeats allowed; None = every graph) of a GraphStore built at
        this model's n_max.  Dropout is off whatever flags.dropout says."""
        self._no_web('embed')
        return self._embed('embed', store, graph_idx)

    def score_grid(self, emb_q, emb_db, final=True):
        """Scores [m][n] of (query i as graph 1, database j as graph 2) from embeddings
        (embed): the similarity (final activation applied) or, final=False, the
        pre-activation score of pred_sim_without_act."""
        self._no_web('score_grid')
        return self._score_grid('score_grid', emb_q, emb_db, final)

    def topk(self, scores, k, largest=True):
        """(idx int32 [m][k], values [m][k]) of the k best entries of each row of scores:
        by value, ties to the smaller column, NaN last."""
        torch = self.torch
        s = torch.as_tensor(scores, dtype=torch.float32, device=self.device)
        if s.dim() != 2:
            raise _lib.SiameseHipError('topk: scores must be [m][n]')
        s = s.contiguous()
        m, n = int(s.shape[0]), int(s.shape[1])
        idx = torch.empty((m, max(int(k), 0)), dtype=torch.int32, device=self.device)
        val = torch.empty((m, max(int(k), 0)), dtype=torch.float32, device=self.device)
        _lib.topk_rows(s, m, n, n, k, largest, idx, val)
        return idx, val

    def search(self, emb_q, emb_db, k, largest=True, final=True, seg_cols=0):
        """(idx int32 [m][k], values [m][k]): topk(score_grid(emb_q, emb_db, final), k,
        largest), bit for bit, from one fused call that never holds the [m][n] scores
        (include/siamese_search.h).  seg_cols: database columns per workgroup, 0 = the
        library's choice; the result does not depend on it."""
        self._no_web('search')
        return self._search('search', emb_q, emb_db, k, largest, final, seg_cols)

    # ---- embed-once retrieval for graph-store models (include/siamese_web_embed.h) ----
    def web_embed(self, store, graph_idx=None):
        """Graph-level embeddings [count][D] (torch, on the device) of the graphs graph_idx
        (store ids, repeats allowed; None = every graph) of a web.CsrStore.  The tensor is a
        view of the [count][ld] buffer the kernel writes (ld = D rounded up to 128): it keeps
        that row stride.  Dropout is off whatever flags.dropout says."""
        self._only_web('web_embed')
        return self._embed('web_embed', store, graph_idx)

    def web_score_grid(self, emb_q, emb_db, final=True):
        """Scores [m][n] of (query i as graph 1, database j as graph 2) from embeddings
        (web_embed, or any 2-D float32 tensors [*, D] with unit inner stride: their row
        strides are passed on): the similarity, or, final=False, the pre-activation score
        of pred_sim_without_act."""
        self._only_web('web_score_grid')
        return self._score_grid('web_score_grid', emb_q, emb_db, final)

    def web_search(self, emb_q, emb_db, k, largest=True, final=True, seg_cols=0):
        """(idx int32 [m][k], values [m][k]): topk(web_score_grid(emb_q, emb_db, final), k,
        largest), bit for bit, from one fused call that never holds the [m][n] scores
        (include/siamese_web_search.h).  Row strides are handled as web_score_grid handles
        them.  seg_cols: database columns per workgroup, 0 = the library's choice; the result
        does not depend on it."""
        self._only_web('web_search')
        return self._search('web_search', emb_q, emb_db, k, largest, final, seg_cols)

    # ---- embed-once training (include/siamese_embed_train.h, siamese_web_embed_train.h:
    # dropout 0 only; include/siamese_embed_drop.h, siamese_web_embed_drop.h: dropout='graph',
    # masks keyed per graph) ----
    def _no_dropout(self, what):
        if self.flags.dropout != 0:
            raise _lib.SiameseHipError(
                '{}: embed-once training needs flags.dropout = 0 (it is {}): the reference '
                'draws its dropout masks per pair, so with dropout on a graph\'s embedding '
                'depends on its partner; use fwd_bwd / train_step, or dropout=\'graph\' '
                '(one mask set per graph per step)'.format(what, self.flags.dropout))

    def _grid_dropout(self, dropout, what):
        """None: today's embed-once training, which refuses flags.dropout != 0; 'graph':
        masks keyed per graph (include/siamese_embed_drop.h)."""
        if dropout is None:
            self._no_dropout(what)
        elif dropout != 'graph':
            raise _lib.SiameseHipError('{}: dropout must be None or \'graph\', not {!r}'.format(
                what, dropout))

    def _sg_keep1(self):
        """A copy of the model struct with keep_prob = 1 (built once): what the grid calls
        take when the head's mask is already in the embeddings."""
        m = getattr(self, '_sg_keep1_copy', None)
        if m is None:
            m = _lib.SgModel.from_buffer_copy(self.sg)
            m.keep_prob = 1.0
            self._sg_keep1_copy = m
        return m

    def _grid_problem(self, what, store, labels, q_idx, db_idx, y_stats, dropout):
        torch, fam = self.torch, self._family
        self._grid_dropout(dropout, what)
        if not fam.web:
            self._check_store_capacity(store)
        self.check_node_counts(store.n, what)
        G = len(store)
        if G == 0 or int(np.asarray(store.n).min()) < 1:
            raise _lib.SiameseHipError('{}: every store graph needs at least one '
                                       'node'.format(what))
        q = np.arange(G) if q_idx is None else np.asarray(q_idx, np.int64).reshape(-1)
        db = np.arange(G) if db_idx is None else np.asarray(db_idx, np.int64).reshape(-1)
        both = np.concatenate([q, db])
        if both.size and (both.min() < 0 or both.max() >= G):
            raise _lib.SiameseHipError('{}: graph ids must lie in [0, {})'.format(what, G))
        uniq, inv = np.unique(both, return_inverse=True)
        m, n, dev = int(q.size), int(db.size), self.device
        lab = torch.as_tensor(labels if torch.is_tensor(labels) else
                              np.asarray(labels, np.float32), dtype=torch.float32,
                              device=dev).contiguous()
        if tuple(lab.shape) != (m, n):
            raise _lib.SiameseHipError('{}: labels must be [{}][{}]'.format(what, m, n))
        if y_stats is None:
            y_stats = _label_stats(torch, lab, m * n)
        ld, U = self._embed_dims()[1], int(uniq.size)
        # graph-store models: the gradient buffers start as zeros, because the kernels leave
        # columns [D, ld) untouched, and the Python store is kept alive beside its struct
        grad = torch.zeros if fam.web else torch.empty
        store_dev = store.to_device(dev)
        bwd_ws = fam.embed_drop_bwd_ws if dropout else fam.embed_bwd_ws
        fwd_ws = fam.embed_drop_ws if dropout else fam.embed_ws
        return GridProblem(
            store_dev=(store, store_dev) if fam.web else store_dev, m=m, n=n, labels=lab,
            y_stats=y_stats, uniq=torch.from_numpy(uniq.astype(np.int32)).to(dev),
            q_pos=torch.from_numpy(inv[:m].astype(np.int64)).to(dev),
            db_pos=torch.from_numpy(inv[m:].astype(np.int64)).to(dev),
            identity=bool(m == n == U and np.array_equal(q, uniq) and np.array_equal(db, uniq)),
            emb=self._f32((U, ld)), g_emb=self._f32((U, ld), grad),
            g_q=self._f32((m, ld), grad), g_db=self._f32((n, ld), grad),
            status=torch.zeros(1, dtype=torch.int32, device=dev),
            ws_grid=self._new_ws(fam.grid_bwd_ws(self._sg_keep1() if dropout else self.sg, m, n)),
            ws_embed=self._new_ws(bwd_ws(self.sg, U)),
            ws_fwd=self._new_ws(fwd_ws(self.sg, U)) if fam.web else None, dropout=dropout)

    def _grid_fwd_bwd(self, what, problem, store, labels, q_idx, db_idx, add_label_term, s_out,
                      dropout, seed):
        """The grid step: embed the distinct graphs, run the grid forward and backward, sum the
        role gradients, run the node-stack backward.  problem: the public *grid_problem."""
        fam = self._family
        if isinstance(store, GridProblem):
            gp = store
            if dropout is not None and dropout != gp.dropout:
                raise _lib.SiameseHipError('{}: dropout={!r} on a {} built with '
                                           'dropout={!r}'.format(what, dropout, problem.__name__,
                                                                 gp.dropout))
            self._grid_dropout(gp.dropout, what)
        else:
            self._grid_dropout(dropout, what)
            gp = problem(store, labels, q_idx, db_idx, dropout=dropout)
        if fam.web and gp.ws_fwd is None:
            raise _lib.SiameseHipError('{}: the problem was built by grid_problem; use '
                                       'web_grid_problem'.format(what))
        store_dev = gp.store_dev[1] if fam.web else gp.store_dev
        U, ld = int(gp.uniq.numel()), int(gp.emb.shape[1])
        # dropout='graph': the step's seed, and for the grid the model with keep_prob 1 (the
        # masks are in the embeddings); the node-stack calls take the model itself
        seed = self._seed(seed) if gp.dropout else None
        sg = self._sg_keep1() if gp.dropout else self.sg
        self._embed_call(store_dev, gp.uniq, U, seed, gp.emb, gp.ws_fwd, gp.status)
        eq, edb = (gp.emb, gp.emb) if gp.identity else (gp.emb[gp.q_pos], gp.emb[gp.db_pos])
        # a head without variables (Dot) takes no params and writes no gradient of its own: the
        # node-stack backward writes all of grad
        head = [self.params] if fam.params else []
        fam.grid_fwd_bwd(sg, *([eq, ld, edb, ld] if fam.strided else [eq, edb]), gp.m, gp.n,
                         *head, gp.labels, gp.n, gp.m * gp.n, gp.y_stats, add_label_term, s_out,
                         gp.n, *([gp.g_q, ld, gp.g_db, ld] if fam.web else [gp.g_q, gp.g_db]),
                         *([self.grad] if fam.params else []), self.loss_buf, gp.ws_grid)
        if gp.identity:
            self.torch.add(gp.g_q, gp.g_db, out=gp.g_emb)
        else:
            gp.g_emb.zero_()
            gp.g_emb.index_add_(0, gp.q_pos, gp.g_q)
            gp.g_emb.index_add_(0, gp.db_pos, gp.g_db)
        (fam.embed_drop_bwd if gp.dropout else fam.embed_bwd)(
            self.sg, *self._node_args(store_dev, gp.uniq, U, seed), gp.g_emb,
            *([ld] if fam.web else []), self.grad, gp.ws_embed, gp.status)
        return gp

    def _grid_train_step(self, fwd_bwd, store, labels, q_idx, db_idx, sync, dropout):
        fwd_bwd(store, labels, q_idx, db_idx, dropout=dropout)
        if self.grad_hook is not None:
            self.grad_hook(self)
        self.apply_adam()
        self.step_count += 1
        if not sync:
            return None
        return float(self.loss_buf[0].item() + self.reg_buf[0].item())

    def grid_problem(self, store: GraphStore, labels, q_idx=None, db_idx=None, y_stats=None,
                     dropout=None):
        """The device-resident state of an m x n block of pairs (query q_idx[i] as graph 1,
        database db_idx[j] as graph 2; None = every store graph) with labels [m][n]: the
        distinct graphs, where each query / database entry sits among them, the labels and
        their {ȳ, ½Σ(y−ȳ)²} (float64, as AllPairsShard), and every buffer a step needs.
        Build once, step many times (grid_fwd_bwd / grid_train_step).
        dropout: None serves flags.dropout = 0 only; 'graph' trains with dropout masks keyed
        per graph (grid_fwd_bwd) and is stored on the problem."""
        self._no_web('grid_problem')
        return self._grid_problem('grid_problem', store, labels, q_idx, db_idx, y_stats, dropout)

    def grid_fwd_bwd(self, store, labels=None, q_idx=None, db_idx=None, add_label_term=True,
                     s_out=None, dropout=None, seed=None):
        """fwd_bwd over the m x n block of pairs, embed-once: every distinct graph's node
        stack runs forward once (sg_embed), the NTN grid runs forward and backward
        (sg_score_grid_fwd_bwd: loss, the head's gradient, the embeddings' gradients), the
        query-role and database-role gradients of each graph are summed and go once through
        its node stack (sg_embed_bwd).  Leaves Σ∂loss_mse/∂θ in self.grad and loss_mse in
        self.loss_buf[0] exactly where fwd_bwd over the m·n pairs (batch_total = m·n) leaves
        them, up to fp32 summation order.  store: a GraphStore with labels [m][n], or a
        grid_problem(...) built once.  s_out: [m][n] pre-activation scores, optional.
        Needs the NTN head the score grid serves, or the Dot head (the grid call is then
        sg_dot_score_grid_fwd_bwd, include/siamese_dot_embed.h: no head variables, the
        node-stack backward writes the whole gradient) and, with dropout=None,
        flags.dropout = 0.

        dropout='graph' (given here, or stored on the grid_problem) trains with dropout,
        the masks keyed per graph: distinct graph c of the step (ascending store id) is
        embedded as side c & 1 of unit c >> 1 under the step's seed (seed, default the
        train steps' seed of step_count), with the node layers' masks and the NTN input mask
        the generic pair kernel draws for that pair and side (sg_embed_drop); the grid runs
        on the masked embeddings with keep_prob 1, and sg_embed_drop_bwd takes the summed
        role gradients back under the same masks.  A graph that is both a query and a
        database entry has ONE mask set per step, in both roles and in every pair.  This is
        ordinary dropout of a batched Siamese model and deviates from the reference, which
        draws fresh masks for every pair (quirk A4): the loss and gradient are not those of
        fwd_bwd over the m·n pairs.  At flags.dropout = 0 it equals dropout=None."""
        if isinstance(store, GridProblem):   # a store is refused by grid_problem, in its place
            self._no_web('grid_fwd_bwd')
        return self._grid_fwd_bwd('grid_fwd_bwd', self.grid_problem, store, labels, q_idx,
                                  db_idx, add_label_term, s_out, dropout, seed)

    def grid_train_step(self, store, labels=None, q_idx=None, db_idx=None, sync=True,
                        dropout=None):
        """grid_fwd_bwd followed by Adam: train_step's embed-once counterpart (same loss
        return: loss_mse + weight decay at the pre-update parameters).  With dropout='graph'
        every step draws new masks (the seed follows step_count)."""
        return self._grid_train_step(self.grid_fwd_bwd, store, labels, q_idx, db_idx, sync,
                                     dropout)

    def web_grid_problem(self, store, labels, q_idx=None, db_idx=None, y_stats=None,
                         dropout=None):
        """grid_problem for a graph-store (Web) model: the device-resident state of an m x n
        block of pairs over a web.CsrStore (query q_idx[i] as graph 1, database db_idx[j] as
        graph 2; None = every store graph) with labels [m][n].  The embedding buffers keep
        the [*][ld] rows of sg_web_embed (ld = D rounded up to 128).  Build once, step many
        times (web_grid_fwd_bwd / web_grid_train_step).
        dropout: None serves flags.dropout = 0 only; 'graph' trains with dropout masks keyed
        per graph (web_grid_fwd_bwd) and is stored on the problem."""
        self._only_web('web_grid_problem')
        return self._grid_problem('web_grid_problem', store, labels, q_idx, db_idx, y_stats,
                                  dropout)

    def web_grid_fwd_bwd(self, store, labels=None, q_idx=None, db_idx=None, add_label_term=True,
                         s_out=None, dropout=None, seed=None):
        """grid_fwd_bwd for a graph-store (Web) model: every distinct graph's CSR node stack
        runs forward once (sg_web_embed), the large-D NTN grid runs forward and backward
        (sg_web_score_grid_fwd_bwd), the query-role and database-role gradients of each graph
        are summed and go once through its node stack (sg_web_embed_bwd).  Leaves
        Σ∂loss_mse/∂θ in self.grad and loss_mse in self.loss_buf[0] where fwd_bwd over the
        m·n pairs (web_batch, batch_total = m·n) leaves them, up to fp32 summation order.
        store: a web.CsrStore with labels [m][n], or a web_grid_problem(...) built once.
        s_out: [m][n] pre-activation scores, optional.  With dropout=None it needs
        flags.dropout = 0.

        dropout='graph' (given here, or stored on the web_grid_problem) trains with dropout,
        the masks keyed per graph exactly as grid_fwd_bwd does for the other paths: distinct
        graph c of the step (ascending store id) is embedded as side c & 1 of unit c >> 1
        under the step's seed (seed, default the train steps' seed of step_count) with the
        masks the pair kernel draws for that pair and side (sg_web_embed_drop); the grid runs
        on the masked embeddings with keep_prob 1, and sg_web_embed_drop_bwd takes the summed
        role gradients back under the same masks.  One mask set per graph per step: not the
        reference's per-pair masks (quirk A4), so the loss and gradient are not those of
        fwd_bwd over the m·n pairs.  At flags.dropout = 0 it equals dropout=None."""
        self._only_web('web_grid_fwd_bwd')
        return self._grid_fwd_bwd('web_grid_fwd_bwd', self.web_grid_problem, store, labels,
                                  q_idx, db_idx, add_label_term, s_out, dropout, seed)

    def web_grid_train_step(self, store, labels=None, q_idx=None, db_idx=None, sync=True,
                            dropout=None):
        """web_grid_fwd_bwd followed by Adam: train_step's embed-once counterpart for
        graph-store models (same loss return: loss_mse + weight decay at the pre-update
        parameters).  With dropout='graph' every step draws new masks (the seed follows
        step_count)."""
        return self._grid_train_step(self.web_grid_fwd_bwd, store, labels, q_idx, db_idx, sync,
                                     dropout)

    def flat_params(self) -> np.ndarray:
        return self.params.detach().cpu().numpy()

    def set_params(self, flat):
        self.params.copy_(self.torch.as_tensor(np.asarray(flat, np.float32)))

    # ---- checkpoint / resume (models.py:118-131 counterpart) -------------------
    def state_dict(self):
        return dict(params=self.params.cpu(), adam_m=self.adam_m.cpu(), adam_v=self.adam_v.cpu(),
                    beta_powers=self.beta_powers.cpu(),
                    step_count=self.torch.tensor(self.step_count))

    def load_state_dict(self, sd):
        self.params.copy_(sd['params'])
        self.adam_m.copy_(sd['adam_m'])
        self.adam_v.copy_(sd['adam_v'])
        self.beta_powers.copy_(sd['beta_powers'])
        self.step_count = int(sd['step_count'])

    def save(self, path):
        self.torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(self.torch.load(path, weights_only=True))


class GraphSteps(object):
    """Captured train steps of SiameseGCNTNMSE (see capture_train_steps)."""

    def __init__(self, model, feed, n_steps: int = 1):
        import torch
        if model.kernel_path != 1:
            raise RuntimeError('graph-captured steps need the fused path (kernel path 1)')
        if model.grad_hook is not None:
            # a data-parallel hook is host-driven (torch.distributed / gloo): it cannot be
            # recorded into a hipGraph, and a replay would silently skip the exchange
            raise RuntimeError('graph-captured steps do not support a grad_hook (the '
                               'all-reduce of a sharded step); run eager train_step instead')
        self.model, self.feed, self.n_steps = model, feed, int(n_steps)
        m = model
        self.seed_dev = torch.tensor([m._seed(None)], dtype=torch.int64, device=m.device)
        ws = m.workspace(feed.B)
        state = self._snapshot()
        # warm-up on a side stream (allocator pools, lazy handles), then restore
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._body(ws)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._restore(state)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for _ in range(self.n_steps):
                self._body(ws)
        torch.cuda.synchronize()
        self._restore(state)   # capture records the work; the state must not move

    def _body(self, ws):
        m = self.model
        b = self.feed.next_batch()
        if m._adam_ws is None:   # reduction + Adam in one launch
            f = m.flags
            _lib.train_step_dseed(m.sg, b.records, b.n_pairs, b.pair_offset, b.batch_total,
                                  m.params, self.seed_dev, b.y_stats, 1, None, m.grad,
                                  m.loss_buf, ws, m.adam_m, m.adam_v, f.learning_rate, m.beta1,
                                  m.beta2, m.eps, f.weight_decay, m.beta_powers, m.reg_buf)
        else:
            _lib.fwd_bwd_dseed(m.sg, b.records, b.n_pairs, b.pair_offset, b.batch_total,
                               m.params, self.seed_dev, b.y_stats, 1, None, m.grad, m.loss_buf,
                               ws)
            m.apply_adam()
        _lib.seed_advance(self.seed_dev, 1)

    def _snapshot(self):
        m, f = self.model, self.feed
        return [t.clone() for t in (m.params, m.adam_m, m.adam_v, m.beta_powers,
                                    f.sampler.state, self.seed_dev)]

    def _restore(self, st):
        m, f = self.model, self.feed
        for dst, src in zip((m.params, m.adam_m, m.adam_v, m.beta_powers, f.sampler.state,
                             self.seed_dev), st):
            dst.copy_(src)

    def replay(self, times: int = 1):
        """Run the captured steps `times` times; leaves the last step's loss_mse in
        model.loss_buf and advances model.step_count like eager steps."""
        for _ in range(int(times)):
            self.graph.replay()
        self.model.step_count += self.n_steps * int(times)


def create_model(model, input_dim, flags=None, **kw):
    """models_factory.py:5-11."""
    if model == 'siamese_gcntn_mse':
        return SiameseGCNTNMSE(input_dim, flags, **kw)
    elif model == 'siamese_gcntn_hinge':
        raise RuntimeError('siamese_gcntn_hinge is an unimplemented stub in the reference '
                           '(model_hinge.py:5-45)')
    raise RuntimeError('Unknown model {}'.format(model))
