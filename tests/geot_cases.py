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
* ``PATHS`` / ``DEFAULTS``: the engine path table of tests/test_gpu_geot_edge_shapes.py and
  tests/test_gpu_geot_saturated.py.
* saturating weights (``SAT_FACTORS``, ``saturating_state_dict``): the seeded state dict with, per
  gt_block, mha_module.Q / K scaled by s_qk and mha_module.edge_feats_projection by s_p (none of them
  has a bias), so that both attention clamps (graph_utils.py:29-32, :58-61) bind on a sizeable share
  of the elements and head sums without the head sums turning into a step function. Calibrated layer
  by layer on ragged300 / general with the fp64 oracle: s_qk = sqrt(5 / q85(|K.Q / sqrt(32)|)), then
  s_p = 5 / q75(|head sum|), rounded to quarters.
* ``mha_variant`` / ``variant64``: a restatement of oracle.mha with three switches (element clamp,
  head-sum clamp, element clamp moved in front of the / sqrt(32)) that records how many pre-clamp
  values lie beyond +-5, swapped in for oracle.mha while a forward runs in float64. ``MUTANTS`` are
  the three wrong clamp placements.
* ``bf16_sensitivity`` / ``bf16_bound``: how far the fp64 reference itself moves when every floating
  parameter and node_f are rounded to bf16, and the bf16 bound that follows from it.
"""
import os

import numpy as np
import torch

from gpu_common import rel_max
from oracle import geot_oracle as O

LAYERS = (1, 2, 3)
TOL = {"f32": 1e-4, "bf16": 1.5e-2}  # BASELINE.json north_star; tests/test_gpu_parity.py

# (dtype, path) -> engine attributes that differ from the defaults
PATHS = {
    ("bf16", "default"): {},
    ("bf16", "f_form"): {"z_init": False},
    ("bf16", "unfused_resident"): {"fuse_embed_init": False},
    ("bf16", "unfused_staged"): {"fuse_embed_init": False, "resident_init": False},
    ("bf16", "fused_node"): {"split_node": False},
    ("bf16", "fold"): {"fold_attn": True},
    ("f32", "default"): {},
    ("f32", "unfused"): {"fuse_embed_init": False},
    ("f32", "fused_node"): {"split_node": False},
}
DEFAULTS = {"z_init": True, "fuse_embed_init": True, "resident_init": True, "split_node": True, "fold_attn": False}

# gt_block index -> (s_qk, s_p); an L-deep state dict takes blocks 0 .. L-1 (block L-1 is the final layer)
SAT_FACTORS = {0: (7.75, 1.75), 1: (4.75, 0.5), 2: (3.0, 0.25)}
# the wrong clamp placements the saturating cases are there to tell from the reference's
MUTANTS = {"no_element_clamp": {"elem_clamp": False}, "no_sum_clamp": {"sum_clamp": False},
           "clamp_before_scale": {"clamp_first": True}}
TAILS = ("elem_lo", "elem_hi", "sum_lo", "sum_hi")
TINY_KNN = ("knn7_k3", "knn11_k3")  # 84 and 132 head sums: too few for a share of them, or for the bf16 bound
# tests/golden/make_golden_saturated.py: the reference's own LitGINI under saturating weights
SAT_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sat_tiny.npz")

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

_items, _sds, _refs, _sat_sds, _sens = {}, {}, {}, {}, {}


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


def scale_attention(sd, factors):
    """A copy of sd with gt_block li's mha_module.Q / K weights times factors[li][0] and its
    edge_feats_projection weight times factors[li][1]; every other tensor shared, unchanged."""
    out = dict(sd)
    for li, (s_qk, s_p) in factors.items():
        p = f"gnn_module.0.gt_block.{li}.mha_module"
        if f"{p}.Q.weight" not in sd:
            continue
        assert not any(f"{p}.{m}.bias" in sd for m in ("Q", "K", "edge_feats_projection"))
        out[f"{p}.Q.weight"], out[f"{p}.K.weight"] = sd[f"{p}.Q.weight"] * s_qk, sd[f"{p}.K.weight"] * s_qk
        out[f"{p}.edge_feats_projection.weight"] = sd[f"{p}.edge_feats_projection.weight"] * s_p
    return out


def saturating_state_dict(num_layers):
    """state_dict(num_layers) with SAT_FACTORS applied, cached."""
    if num_layers not in _sat_sds:
        _sat_sds[num_layers] = scale_attention(state_dict(num_layers), SAT_FACTORS)
    return _sat_sds[num_layers]


def mha_variant(elem_clamp=True, sum_clamp=True, clamp_first=False, tails=None):
    """oracle.mha restated, in the dtype of its inputs, with the clamps switchable. The defaults are
    the reference's placement, op for op what oracle.mha does. tails: a list that receives one dict
    per call with the numbers of elements / head sums and how many of the values the REFERENCE would
    clamp (K.Q / sqrt(32) per element; the head sum as this variant computes it) lie below -5 / above 5."""
    def mha(sd, p, g, node, edge, update_edge_feats):
        src, dst, N = g["src"], g["dst"], g["num_nodes"]
        Q = O._lin(node, sd, f"{p}.Q").view(-1, O.HEADS, O.DH)
        K = O._lin(node, sd, f"{p}.K").view(-1, O.HEADS, O.DH)
        V = O._lin(node, sd, f"{p}.V").view(-1, O.HEADS, O.DH)
        P = O._lin(edge, sd, f"{p}.edge_feats_projection").view(-1, O.HEADS, O.DH)
        score = K[src] * Q[dst]
        pre = score / np.sqrt(O.DH)
        if clamp_first:
            score = score.clamp(-5.0, 5.0) / np.sqrt(O.DH)
        else:
            score = pre.clamp(-5.0, 5.0) if elem_clamp else pre
        score = score * P
        e_out = score if update_edge_feats else None
        total = score.sum(-1, keepdim=True)
        if tails is not None:
            tails.append({"layer": p, "elems": pre.numel(), "sums": total.numel(),
                          "elem_lo": int((pre < -5).sum()), "elem_hi": int((pre > 5).sum()),
                          "sum_lo": int((total < -5).sum()), "sum_hi": int((total > 5).sum())})
        score = torch.exp(total.clamp(-5.0, 5.0) if sum_clamp else total)
        wV = torch.zeros(N, O.HEADS, O.DH).index_add_(0, dst, V[src] * score)
        z = torch.zeros(N, O.HEADS, 1).index_add_(0, dst, score)
        h = wV / (z + torch.full_like(z, 1e-6))
        return h, e_out
    return mha


def tail_fractions(t):
    """The four tail fractions of one mha_variant record, in TAILS' order."""
    return tuple(t[k] / t["elems" if k.startswith("elem") else "sums"] for k in TAILS)


def variant64(forward, sd, item, num_layers, **switches):
    """forward (oracle.geot_forward, plain_cases.plain_forward) in float64 with mha_variant(**switches)
    in oracle.mha's place (restored afterwards) -> (node, edge, [tail record per layer]), and the
    forward's intermediates as a fourth with return_intermediates=True. fp32=True: in float32 instead."""
    return_intermediates, fp32 = switches.pop("return_intermediates", False), switches.pop("fp32", False)
    tails, prev = [], O.mha
    O.mha = mha_variant(tails=tails, **switches)
    try:
        if fp32:
            with torch.no_grad():
                node, edge, inter = forward(sd, item, num_layers, True)
        else:
            node, edge, inter = in_fp64(forward, to64(sd), to64(item), num_layers, True)
    finally:
        O.mha = prev
    assert len(tails) == num_layers
    out = (node.numpy(), edge.numpy(), tails)
    return out + ({k: v.numpy() for k, v in inter.items()},) if return_intermediates else out


def bf16_sensitivity(sd, item, num_layers, key=None, forward=None):
    """(node, edge) rel_max of the float64 forward with every floating parameter and node_f rounded to
    bf16 against the unrounded float64 run: how far the reference itself moves under the rounding a
    bf16 engine starts from. Cached per (key, num_layers) when a key is given."""
    if key is not None and (key, num_layers) in _sens:
        return _sens[key, num_layers]
    forward = forward or O.geot_forward
    # bf16 keeps 8 significant bits: round-to-nearest-even of every value, the cast the engines start from
    rnd = lambda t: t.bfloat16().to(t.dtype) if torch.is_tensor(t) and t.is_floating_point() else t  # noqa: E731
    exact = in_fp64(forward, to64(sd), to64(item), num_layers)
    moved = in_fp64(forward, to64({k: rnd(v) for k, v in sd.items()}), to64(dict(item, node_f=rnd(item["node_f"]))),
                    num_layers)
    out = tuple(rel_max(m.numpy(), x.numpy()) for m, x in zip(moved, exact))
    if key is not None:
        _sens[key, num_layers] = out
    return out


def bf16_bound(sens_saturating, sens_seeded):
    """The project's bf16 budget scaled by how much more the reference moves under bf16 rounding with
    the saturating weights than with the seeded ones; never below the budget itself."""
    return TOL["bf16"] * max(1.0, sens_saturating / sens_seeded)


def sat_bounds(dtype, sens_saturating=None, sens_seeded=None):
    """(node bound, edge bound) of one chain under saturating weights: fp32 the project's 1e-4, bf16
    bf16_bound of that chain's two (node, edge) sensitivities."""
    if dtype == "f32":
        return TOL["f32"], TOL["f32"]
    return tuple(bf16_bound(a, b) for a, b in zip(sens_saturating, sens_seeded))


def check_tail_window(name, tails):
    """Every layer's four tails hold 1 % .. 40 % of their elements; for the tiny kNN chains, at least
    one element each."""
    for t in tails:
        for k, frac in zip(TAILS, tail_fractions(t)):
            if name in TINY_KNN:
                assert t[k] >= 1, (name, t["layer"], k, t)
            else:
                assert 0.01 <= frac <= 0.40, (name, t["layer"], k, frac, t)


def mutant_errors(forward, sd, item, num_layers, ref):
    """mutant name -> (node, edge) rel_max of the mutant's float64 run against ref = (node, edge)."""
    out = {}
    for m, switches in MUTANTS.items():
        node, edge, _ = variant64(forward, sd, item, num_layers, **switches)
        out[m] = (rel_max(node, ref[0]), rel_max(edge, ref[1]))
    return out


def check_decisive(name, errors, bf16_bounds):
    """Each mutant misses the reference by more than twice the GPU bound on the node or the edge
    output: in both dtypes, in fp32 alone for the tiny kNN chains."""
    for m, (en, ee) in errors.items():
        for dtype in ("f32",) if name in TINY_KNN else ("f32", "bf16"):
            bn, be = sat_bounds("f32") if dtype == "f32" else bf16_bounds
            assert en > 2 * bn or ee > 2 * be, (name, m, dtype, (en, ee), (bn, be))


def fixture_item(z, tag):
    """Chain g1 / g2 of a fixture as a from_arrays / oracle item."""
    t = lambda name, dt: torch.as_tensor(z[f"{tag}_{name}"].astype(dt))  # noqa: E731
    return {"num_nodes": int(z[f"{tag}_node_f"].shape[0]), "src": t("src", np.int64), "dst": t("dst", np.int64),
            "src_nbr": t("src_nbr", np.int64), "dst_nbr": t("dst_nbr", np.int64),
            "node_f": t("node_f", np.float32), "edge_f": t("edge_f", np.float32)}


def sat_stage_errors(z, mode, tag, node, edge, inter, colsums=True):
    """stage -> rel_max of one chain's outputs against sat_tiny.npz's (mode "geo" / "plain"): the node
    stages in full, the edge stages at the stored rows (the chain's last among them), whose float64
    column sums over all rows must agree as well (colsums=False: not asserted, for a mutant)."""
    errs = {}
    for name, got in (("node_out", node), ("layer0_node", inter["node0"])):
        errs[name] = rel_max(got, z[f"{mode}_{tag}_{name}"])
    for name, got, rname in (("init_edge", inter["init_edge"], "init_edge_rows"),
                             ("layer0_edge", inter["edge0"], "layer0_edge_rows"), ("edge_out", edge, "edge_rows")):
        rows = z[f"{mode}_{tag}_{rname}"]
        got = np.asarray(got, dtype=np.float64)
        assert rows[-1] == got.shape[0] - 1
        if colsums:
            assert np.abs(got.sum(0) - z[f"{mode}_{tag}_{name}_colsum"]).max() <= 1e-5 * np.abs(got).sum(0).max(), name
        errs[name] = rel_max(got[rows], z[f"{mode}_{tag}_{name}"])
    return errs


def sat_stage_errors_unchecked(z, mode, tag, node, edge, inter):
    return sat_stage_errors(z, mode, tag, node, edge, inter, colsums=False)
