"""Shared pieces of the disable_geometric_mode tests (tests/test_plain_host.py on the CPU,
tests/test_gpu_plain.py on the GPU). No tests here.

* ``plain_forward``: the plain Graph Transformer's GeoT forward for ONE chain, restated from
  oracle.geot_oracle's own functions (_lin, _bn, mha) without touching oracle/: what
  DGLGeometricTransformer.forward computes with disable_geometric_mode
  (deepinteract_modules.py:1444-1451, :676, :897-904), in the dtype of its inputs.
* ``plain_forward64``: the same in float64 (geot_cases.in_fp64 / to64), cached per (key, layers).
* ``state_dict``: seeded_state_dict(seed, default 0) of a plain GeoT of L layers, without the head.
* saturating weights (``SAT_SEED``, ``SAT_FACTORS``, ``saturating_state_dict``, ``variant64``,
  ``bf16_sensitivity``): geot_cases' treatment of the attention clamps for this mode, with a weight
  seed and factors of its own (see SAT_FACTORS).
* ``fixture``: tests/golden/plain_tiny.npz (tests/golden/make_golden_plain.py: the reference's own
  LitGINI(disable_geometric_mode=True) on a 33 + 21 residue complex).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import geot_cases as C
from oracle import geot_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plain_tiny.npz")
# gt_block index -> ((s_qk, s_p) as an intermediate layer, (s_qk, s_p) as the final layer). In this mode
# the final layer's projection reads the 30-wide conformation Linear's output, not the hidden edge
# features, so its head sums have a scale of their own: block L-1 of an L-deep state dict takes the
# second pair. geot_cases' recipe (q85 / q75 on ragged300) leaves the kNN chains' final layers with
# under 1 % of their head sums beyond +-5, so the pairs were chosen layer by layer (earlier blocks
# fixed, each role at its own depth) over all the non-tiny chains of tests/test_plain_host.py's
# SAT_CASES: among the quarter-valued pairs that put every tail at 2 % or more and none above 40 %,
# the pair whose largest tail is smallest.
SAT_FACTORS = {0: ((10.0, 0.75), (11.75, 1.0)), 1: ((6.25, 0.25), (6.0, 0.75)), 2: (None, (4.25, 1.0))}
# the weight seed of the saturating cases: with seed 0 the final layer's head sums lean so far to one
# side that no pair of factors puts both of their tails inside tests/test_plain_host.py's window
SAT_SEED = 1
_sds, _refs, _sat_sds = {}, {}, {}


def plain_cfg(num_layers=2, **kw):
    from deepinteract_amd.config import GeoTConfig
    return GeoTConfig(num_gnn_layers=num_layers, disable_geometric_mode=True, **kw)


def state_dict(num_layers, seed=0):
    if (num_layers, seed) not in _sds:
        from deepinteract_amd.weights import seeded_state_dict
        _sds[num_layers, seed] = seeded_state_dict(seed, plain_cfg(num_layers), with_head=False)
    return _sds[num_layers, seed]


def block_factors(num_layers):
    """gt_block index -> (s_qk, s_p) of an L-deep plain state dict."""
    return {li: SAT_FACTORS[li][li == num_layers - 1] for li in range(num_layers)}


def saturating_state_dict(num_layers):
    if num_layers not in _sat_sds:
        _sat_sds[num_layers] = C.scale_attention(state_dict(num_layers, SAT_SEED), block_factors(num_layers))
    return _sat_sds[num_layers]


def variant64(sd, item, num_layers, **switches):
    """geot_cases.variant64 around plain_forward -> (node, edge, [tail record per layer])."""
    return C.variant64(plain_forward, sd, item, num_layers, **switches)


def bf16_sensitivity(sd, item, num_layers, key=None):
    return C.bf16_sensitivity(sd, item, num_layers, key=None if key is None else ("plain", key), forward=plain_forward)


def _cat30(first_two, G):
    return torch.cat((first_two[:, 0].reshape(-1, 1), first_two[:, 1].reshape(-1, 1), G), dim=1)


def _node_side(sd, p, node, h):
    n = node + O._lin(h.reshape(-1, O.H), sd, f"{p}.O_node_feats")
    return n + O._lin(F.silu(O._lin(O._bn(n, sd, f"{p}.batch_norm2_node_feats"), sd, f"{p}.node_feats_MLP.0")),
                      sd, f"{p}.node_feats_MLP.3")


def plain_forward(sd, g, num_layers=2, return_intermediates=False):
    """-> node [N,128], edge [E,128] (the last intermediate layer's edges; InitEdge's when L = 1)."""
    inter = {}
    G = g["edge_f"]
    node = O._lin(g["node_f"], sd, "node_in_embedding")
    edge = O._lin(_cat30(G, G), sd, "gnn_module.0.init_edge_module")          # :1444-1451
    inter["node_emb"], inter["init_edge"] = node, edge
    for li in range(num_layers):
        p = f"gnn_module.0.gt_block.{li}"
        final = li == num_layers - 1
        # the final layer's 30-wide Linear reads columns 0 / 1 of the HIDDEN edge features (:898-903)
        c = O._lin(_cat30(edge, G), sd, f"{p}.conformation_module") if final else edge   # :676
        h, e_out = O.mha(sd, f"{p}.mha_module", g, O._bn(node, sd, f"{p}.batch_norm1_node_feats"),
                         O._bn(c, sd, f"{p}.batch_norm1_edge_feats"), update_edge_feats=not final)
        node = _node_side(sd, p, node, h)
        if not final:
            e = edge + O._lin(e_out.reshape(-1, O.H), sd, f"{p}.O_edge_feats")
            edge = e + O._lin(F.silu(O._lin(O._bn(e, sd, f"{p}.batch_norm2_edge_feats"), sd, f"{p}.edge_feats_MLP.0")),
                              sd, f"{p}.edge_feats_MLP.3")
            inter[f"node{li}"], inter[f"edge{li}"] = node, edge
    if return_intermediates:
        return node, edge, inter
    return node, edge


def plain_forward64(sd, item, num_layers, key=None, return_intermediates=False):
    """float64 numpy results of plain_forward; cached per (key, num_layers), read-only."""
    if key is not None and (key, num_layers) in _refs:
        out = _refs[key, num_layers]
    else:
        node, edge, inter = C.in_fp64(plain_forward, C.to64(sd), C.to64(item), num_layers, True)
        assert node.dtype == torch.float64 and edge.dtype == torch.float64
        out = (node.numpy(), edge.numpy(), {k: v.numpy() for k, v in inter.items()})
        for a in (out[0], out[1], *out[2].values()):
            a.setflags(write=False)
        if key is not None:
            _refs[key, num_layers] = out
    return out if return_intermediates else out[:2]


def fixture():
    return np.load(GOLDEN)


def fixture_item(z, tag):
    """Chain g1 / g2 of the fixture as a from_arrays / oracle item."""
    t = lambda name, dt: torch.as_tensor(z[f"{tag}_{name}"].astype(dt))  # noqa: E731
    return {"num_nodes": int(z[f"{tag}_node_f"].shape[0]), "src": t("src", np.int64), "dst": t("dst", np.int64),
            "src_nbr": t("src_nbr", np.int64), "dst_nbr": t("dst_nbr", np.int64),
            "node_f": t("node_f", np.float32), "edge_f": t("edge_f", np.float32)}
