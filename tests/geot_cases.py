"""Shared cases for the GeoT engine's fp64 comparisons (tests/test_geot_cases_host.py on the CPU,
tests/test_gpu_geot_edge_shapes.py and tests/test_gpu_modules_ragged.py on the GPU). No tests here.

* ``oracle64``: oracle.geot_oracle.geot_forward evaluated in float64 (state dict and inputs cast to
  double, torch's default dtype switched for the call so the oracle's own torch.zeros accumulators are
  double too), cached per (case key, num_layers).
* hand-made ragged chains (``ragged_item``) as GraphBatch.from_arrays items: destination-major edges,
  src uniform over the chain (self-loops and duplicate edges occur), neighbour-edge ids uniform over
  the chain's own edges, node_f / edge_f uniform [0, 1); in two featurisations of edge_f[:, 20:27]:
  "geo_ref" (the reference featuriser's constants, so the DI_GRAPH_GEO_REF kernels apply) and
  "general" (normal direction, normalised normal quaternion).
    ragged37    37 nodes, in-degrees [0,1,8,9,17,40,31,32,33,16] then 0..8:  300 edges (256 + 44)
    ragged300   300 nodes, in-degrees [0,1,16,17,40,100] then 0..12:         1847 edges
    sparse2304  2304 nodes (NODE_COUNT_LIMIT), in-degree 0 except nodes 0 (3), 7 (1), 1152 (33),
                2303 (5): 42 edges, the first and the last with src = 2303, so node_pos reaches the
                last row of InitEdge's positional table
  The ragged batch is [ragged37, sparse2304, ragged300]: the middle chain shifts the third chain's
  node and edge offsets by 2341 and 342 (no multiple of 16, 32 or 256), Et = 2189.
* kNN batches (``KNN_BATCHES``): synth.synthetic_chain chains as tests/test_gpu_wide_rows.py builds
  them; ``knn_host_item`` is the same chain featurised on the CPU by oracle.build_graph.
* ``check``: gpu_common.rel_max plus the row of the worst element.
"""
import numpy as np
import torch

from gpu_common import rel_max
from oracle import geot_oracle as O

LAYERS = (1, 2, 3)
TOL = {"f32": 1e-4, "bf16": 1.5e-2}  # BASELINE.json north_star; tests/test_gpu_parity.py

# name -> (nodes, leading in-degrees, largest drawn in-degree, seed, edges). The seeds are the first
# that give these edge counts; tests/test_geot_cases_host.py holds the conditions a new seed must keep
# (edge counts off multiples of 32, no small reference row, neighbouring last edge rows unlike)
RAGGED = {
    "ragged37": (37, [0, 1, 8, 9, 17, 40, 31, 32, 33, 16], 8, 5, 300),
    "ragged300": (300, [0, 1, 16, 17, 40, 100], 12, 6, 1847),
}
SPARSE_DEG = {0: 3, 7: 1, 1152: 33, 2303: 5}
SPARSE_SEED = 0
RAGGED_BATCH = ("ragged37", "sparse2304", "ragged300")
FEATS = ("geo_ref", "general")

# name -> (chain sizes, k, edges); chain i is synthetic_chain(n, 8100 + i), neighbour seed i + 1
KNN_BATCHES = {"knn7_k3": ([7], 3, 21), "knn11_k3": ([11], 3, 33), "knn21_k20": ([21], 20, 420),
               "knn20_21_k20": ([20, 21], 20, 820)}

_items, _sds, _refs = {}, {}, {}


def _degrees(name):
    if name == "sparse2304":
        deg = torch.zeros(2304, dtype=torch.long)
        for v, d in SPARSE_DEG.items():
            deg[v] = d
        return deg, torch.Generator().manual_seed(SPARSE_SEED), 42
    n, head, hi, seed, edges = RAGGED[name]
    gen = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, hi + 1, (n,), generator=gen)
    deg[:len(head)] = torch.tensor(head)
    return deg, gen, edges


def ragged_item(name, feats):
    """One hand-made chain as a from_arrays item (cached; treat as read-only)."""
    assert feats in FEATS
    if (name, feats) in _items:
        return _items[name, feats]
    from deepinteract_amd.graph import GEO_REF_VALUES
    deg, gen, edges = _degrees(name)
    n, E = deg.numel(), int(deg.sum())
    assert E == edges, (name, E)
    src = torch.randint(0, n, (E,), generator=gen)
    if name == "sparse2304":
        src[0] = src[-1] = n - 1
    base = {"num_nodes": n, "src": src, "dst": torch.repeat_interleave(torch.arange(n), deg),
            "src_nbr": torch.randint(0, E, (E, 2), generator=gen), "dst_nbr": torch.randint(0, E, (E, 2), generator=gen),
            "node_f": torch.rand(n, 113, generator=gen)}
    edge_f = torch.rand(E, 28, generator=gen)
    direction = torch.randn(E, 3, generator=gen)
    quat = torch.nn.functional.normalize(torch.randn(E, 4, generator=gen), dim=1)
    for f in FEATS:
        ef = edge_f.clone()
        ef[:, 20:27] = torch.tensor(GEO_REF_VALUES) if f == "geo_ref" else torch.cat([direction, quat], 1)
        _items[name, f] = dict(base, edge_f=ef)
    return _items[name, feats]


def ragged_batch_items(feats):
    return [ragged_item(name, feats) for name in RAGGED_BATCH]


def knn_chains(name):
    from deepinteract_amd import synth
    sizes, k, _ = KNN_BATCHES[name]
    return [synth.synthetic_chain(n, 8100 + i) for i, n in enumerate(sizes)], k, list(range(1, len(sizes) + 1))


def knn_host_item(name, g):
    """Chain g of a kNN batch, featurised on the CPU (oracle.build_graph, the same neighbour seed)."""
    if (name, g) not in _items:
        chains, k, seeds = knn_chains(name)
        it = O.build_graph(chains[g], k=k, seed=seeds[g])
        _items[name, g] = {key: it[key] for key in ("num_nodes", "src", "dst", "src_nbr", "dst_nbr", "node_f", "edge_f")}
    return _items[name, g]


def host_cases():
    """name -> list of per-chain items, every case the GPU file runs, built on the CPU."""
    cases = {f"ragged_{f}": ragged_batch_items(f) for f in FEATS}
    for name, (sizes, _, _) in KNN_BATCHES.items():
        cases[name] = [knn_host_item(name, g) for g in range(len(sizes))]
    return cases


def oracle_item(gb, g):
    """Chain g of a GraphBatch as the oracle's per-chain item (chain-local ids, CPU tensors)."""
    n0, n1 = gb.node_off[g], gb.node_off[g + 1]
    e0, e1 = gb.edge_off[g], gb.edge_off[g + 1]
    nbr = gb.nbr[e0:e1].long().cpu() - e0
    return {"num_nodes": n1 - n0, "src": gb.src[e0:e1].long().cpu() - n0, "dst": gb.dst[e0:e1].long().cpu() - n0,
            "src_nbr": nbr[:, :2], "dst_nbr": nbr[:, 2:], "node_f": gb.node_f[n0:n1].cpu(),
            "edge_f": gb.edge_f[e0:e1].cpu()}


def state_dict(num_layers):
    """seeded_state_dict(0) of a num_layers-deep GeoT (no head), cached."""
    if num_layers not in _sds:
        from deepinteract_amd.config import GeoTConfig
        from deepinteract_amd.weights import seeded_state_dict
        _sds[num_layers] = seeded_state_dict(0, GeoTConfig(num_gnn_layers=num_layers), with_head=False)
    return _sds[num_layers]


def to64(x):
    """Floating-point tensors (of a dict, too) as double; everything else unchanged."""
    if isinstance(x, dict):
        return {k: to64(v) for k, v in x.items()}
    return x.double() if torch.is_tensor(x) and x.is_floating_point() else x


def in_fp64(fn, *args):
    """fn(*args) under float64 as torch's default dtype (restored afterwards), without autograd."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            return fn(*args)
    finally:
        torch.set_default_dtype(prev)


def oracle64(sd, item, num_layers, key=None):
    """(node [n,128], edge [E,128]) float64 numpy arrays of oracle.geot_forward run in float64.
    key: a hashable name of `item`; results are cached per (key, num_layers) and shared, unchanged,
    by every test that names the same case."""
    if key is not None and (key, num_layers) in _refs:
        return _refs[key, num_layers]
    node, edge = in_fp64(O.geot_forward, to64(sd), to64(item), num_layers)
    assert node.dtype == torch.float64 and edge.dtype == torch.float64
    out = (node.numpy(), edge.numpy())
    for a in out:
        a.setflags(write=False)
    if key is not None:
        _refs[key, num_layers] = out
    return out


def oracle32(sd, item, num_layers):
    with torch.no_grad():
        node, edge = O.geot_forward(sd, item, num_layers)
    return node.numpy(), edge.numpy()


def check(got, ref64, tol=None):
    """(rel_max(got, ref64), row of the worst element). With a tolerance, asserts the error is within
    it (a NaN fails) and names that row."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = rel_max(got, ref)
    diff = np.abs(got - ref).reshape(ref.shape[0], -1)
    row = int(np.argmax(np.where(np.isnan(diff), np.inf, diff).max(axis=1)))
    if tol is not None:
        assert err <= tol, f"rel_max {err:.3e} > {tol:.1e}, worst row {row} of {ref.shape[0]}"
    return err, row
