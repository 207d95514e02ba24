"""Graph sets the MCS tests of _mcs_cases.py never draw (test_mcs_classes_host.py proves on the
host what test_gpu_mcs_classes.py relies on): the graph classes of _ged_classes.py, two sets of
32-node graphs that fill a state's 32 class slots, and stores of capacity 1, 2, 3, 17 and 31;
each with a McsGridReference, and with oracles that need no restatement.

  edge0, forest, dense, densepm, types29, planted9/12/15/16
            _ged_classes.py's graphs and stores (capacity 32 for edge0, 16 for the rest)
  wide32    capacity 32, 32 type names, all distinct within a graph: a 32-node _random_graph g,
            pi(g) under _ged_classes._permuted, pi(g) minus its lowest-degree node, pi(g) plus
            one edge.  g against pi(g) has 32 root classes and maps a node per level: 32
            classes in one state, level 31, in 32 expansions
  wide32k8  the same four graphs with types drawn from 8 names: the 8 root classes split to 16
            and more
  capN      N in (1, 2, 3, 17, 31): a store of that capacity, two types, node counts CAP_SIZES
            (1 and N among them).  The graphs of cap17 and cap31 are prefixes of one
            _random_graph, each under its own node permutation, so the large ones stay alike
            and prove cheaply

MAX_NEED is the largest expansion count the restatement needs to prove a pair of the set, with
an unlimited budget, over all ordered pairs and both `connected` values, measured on the host
with tests/_mcs_restatement.py; PROVE_BUDGET is _ged_classes.budget_for of it, the smallest power
of two at least twice the need (the rule _mcs_cases.PROVE_BUDGET follows).
test_mcs_classes_host.py re-derives both.

  set        need  budget        set        need  budget
  edge0       277     1024       wide32       32      64
  forest       90      256       wide32k8      32      64
  dense      3628     8192       cap1          1       2
  densepm    3628     8192       cap2          2       4
  types29      27       64       cap3          3       8
  planted9     10       32       cap17       1510    4096
  planted12    13       32       cap31      15066   32768
  planted15    16       32
  planted16    16       32

dense and densepm are measured under a cap of DENSE_CAP = 20,000 expansions a pair: the ordered
pairs of ALLOWED_UNPROVEN (K_16 against K_16 minus an edge or a perfect matching, and the two
nearly complete graphs against each other) are still unproven there at both `connected` values,
and 3628 is the largest need of the others.  They are the cut-off cases of these sets: they run
at PROVE_BUDGET like the rest and are compared with the restatement.
"""
import networkx as nx
import numpy as np

import _ged_classes as K
import _mcs_restatement as X
from _ged_exact_cases import _random_graph

GED_SETS = K.SETS
WIDE = ('wide32', 'wide32k8')
CAPS = ('cap1', 'cap2', 'cap3', 'cap17', 'cap31')
SETS = GED_SETS + WIDE + CAPS
TYPES32 = tuple('W{:02d}'.format(i) for i in range(32))
WIDE_K8 = 8                           # type names of wide32k8
WIDE_SEED = 760                       # both wide sets: the same four graphs but for the types
WIDE_P_EXTRA = 0.08
CAP_SIZES = {'cap1': (1, 1, 1, 1), 'cap2': (1, 2, 2, 1, 2), 'cap3': (1, 2, 3, 3, 2, 3),
             'cap17': (1, 5, 17, 17, 16, 12), 'cap31': (1, 8, 31, 31, 30, 24)}
CAP_SEEDS = {'cap1': 771, 'cap2': 772, 'cap3': 773, 'cap17': 774, 'cap31': 775}
CAP_P_EXTRA = 0.08

CUT_BUDGETS = (0, 1, 7)
DENSE_CAP = 20000
ALLOWED_UNPROVEN = {'dense': ((3, 4),),
                    'densepm': ((1, 2), (1, 3), (2, 1), (2, 3), (3, 2))}
MAX_NEED = {'edge0': 277, 'forest': 90, 'dense': 3628, 'densepm': 3628, 'types29': 27,
            'planted9': 10, 'planted12': 13, 'planted15': 16, 'planted16': 16,
            'wide32': 32, 'wide32k8': 32, 'cap1': 1, 'cap2': 2, 'cap3': 3, 'cap17': 1510,
            'cap31': 15066}
PROVE_BUDGET = {name: K.budget_for(need) for name, need in MAX_NEED.items()}

# relabels and edge edits that separate a graph from pi(g), by graph (a leaf or a dropped node
# is no such edit: the smaller graph stays an induced subgraph).  The planted edits build on
# each other, so |difference| separates two of them; the wide graphs 2 and 3 are edited from
# pi(g) each on its own, so the sum does
PLANTED_EDITS = (0, 0, 1, 2, 2)
WIDE_EDITS = (0, 0, 0, 1)


def budgets(name):
    """The budgets the GPU test runs a set at."""
    return CUT_BUDGETS + (PROVE_BUDGET[name],)


def _wide(name):
    """Structure and permutations are drawn before any type, so both sets hold the same four
    graphs."""
    rng = np.random.default_rng(WIDE_SEED)
    g = _random_graph(rng, 32, 0, types=TYPES32, p_extra=WIDE_P_EXTRA)
    order = [int(x) for x in rng.permutation(32)]
    drawn = [int(x) for x in rng.integers(0, WIDE_K8, size=32)]
    for v in range(32):
        g.nodes[v]['type'] = TYPES32[order[v]] if name == 'wide32' else TYPES32[drawn[v]]
    pg, perm = K._permuted(rng, g, 1)
    low = min(range(32), key=lambda v: (pg.degree(v), v))
    keep = [v for v in range(32) if v != low]
    less = nx.Graph(gid=2)
    for i, v in enumerate(keep):
        less.add_node(i, type=pg.nodes[v]['type'])
    less.add_edges_from((keep.index(a), keep.index(b)) for a, b in pg.edges() if low not in (a, b))
    more = nx.Graph(pg, gid=3)
    free = sorted(nx.non_edges(more))
    more.add_edge(*free[int(rng.integers(0, len(free)))])
    return [g, pg, less, more], perm


def _cap(name):
    rng = np.random.default_rng(CAP_SEEDS[name])
    sizes = CAP_SIZES[name]
    base = _random_graph(rng, max(sizes), 0, types=K.TYPES[:2], p_extra=CAP_P_EXTRA)
    out = []
    for gid, n in enumerate(sizes):
        g = nx.Graph(base.subgraph(range(n)), gid=gid)
        if gid % 2 and n <= 3:                       # the small stores: the other type too
            g.nodes[n - 1]['type'] = K.TYPES[1 - K.TYPES.index(g.nodes[n - 1]['type'])]
        out.append(K._permuted(rng, g, gid)[0])
    return out, None


_GRAPHS = {}


def graphs(name):
    if name in GED_SETS:
        return K.graphs(name)
    if name not in _GRAPHS:
        _GRAPHS[name] = _wide(name) if name in WIDE else _cap(name)
    return _GRAPHS[name][0]


def permutation(name):
    """perm of a planted or wide set: node v of graph 0 is node perm[v] of graph 1."""
    if name in GED_SETS:
        return K.permutation(name)
    graphs(name)
    return _GRAPHS[name][1]


def capacity(name):
    if name in GED_SETS:
        return K.capacity(name)
    return 32 if name in WIDE else int(name[len('cap'):])


_STORES = {}


def store(name):
    """(store, McsGridReference) of a named set, built once per process."""
    if name not in _STORES:
        if name in GED_SETS:
            s = K.store(name)[0]
        else:
            from graphembedding_amd.ged import store_of_graphs
            s = store_of_graphs(graphs(name), n_max=capacity(name))
        assert s.n_max == capacity(name)
        _STORES[name] = (s, X.McsGridReference(s))
    return _STORES[name]


# ---- the oracles ----------------------------------------------------------------------------
def _type_counts(g):
    out = {}
    for t in nx.get_node_attributes(g, 'type').values():
        out[t] = out.get(t, 0) + 1
    return out


def common_types(g1, g2):
    """|multiset intersection of the types|: the root's bound ub0."""
    t1, t2 = _type_counts(g1), _type_counts(g2)
    return sum(min(c, t2.get(t, 0)) for t, c in t1.items())


def known(name):
    """{(a, b, connected): ('eq' | 'ge' | 'le', value)} over ordered pairs of a set: what is
    known of the size of the maximum common induced subgraph without a solver.  Pairs without
    an entry have no closed form."""
    gs = graphs(name)
    G = len(gs)
    n = [g.number_of_nodes() for g in gs]
    out = {}
    for a in range(G):                               # a graph against itself
        out[(a, a, 0)] = ('eq', n[a])
        if nx.is_connected(gs[a]):
            out[(a, a, 1)] = ('eq', n[a])
    if name == 'edge0':
        for a in range(G):
            for b in range(G):
                both = common_types(gs[a], gs[b])
                out[(a, b, 0)] = ('eq', both)
                out[(a, b, 1)] = ('eq', min(both, 1))
    elif name in K.DENSE:
        # a clique of K_16 minus k disjoint edges takes one end of each: at most 16 - k nodes
        for a, (na, ma) in enumerate(K.DENSE[name]):
            for b, (nb, mb) in enumerate(K.DENSE[name]):
                if 0 in (ma, mb):
                    size = min(na, nb) if ma == mb else min(na if mb else nb, 16 - ma - mb)
                    out[(a, b, 0)] = out[(a, b, 1)] = ('eq', size)
    elif name in K.PLANTED or name in WIDE:
        edits = PLANTED_EDITS if name in K.PLANTED else WIDE_EDITS
        for a in range(G):
            for b in range(G):
                if a == b:
                    continue
                if a < 2 and b < 2:                  # g against pi(g)
                    out[(a, b, 0)] = out[(a, b, 1)] = ('eq', n[a])
                    continue
                apart = abs(edits[a] - edits[b]) if name in K.PLANTED else edits[a] + edits[b]
                out[(a, b, 0)] = ('ge', min(n[a], n[b]) - apart)
    elif name == 'forest':
        for a in range(7):
            for b in range(7):
                out[(a, b, 0)] = ('eq', min(n[a], n[b]))
    return out


def holds(rule, size, proven=True):
    """An unproven size is a lower bound: it only has to stay at or below a known value."""
    kind, v = rule
    if not proven:
        return kind == 'ge' or size <= v
    return size == v if kind == 'eq' else size >= v if kind == 'ge' else size <= v


def proving_needs(name, cap=None):
    """{(a, b, connected): (proven, expansions)} of the restatement over all ordered pairs of a
    set and both `connected` values, with an unlimited budget or under `cap`."""
    s, ref = store(name)
    G = len(s)
    out = {}
    for a in range(G):
        for b in range(G):
            for c in (0, 1):
                size, bound, _, _, ex = ref.pair(a, b, bool(c), cap)
                out[(a, b, c)] = (size == bound, ex)
    return out
