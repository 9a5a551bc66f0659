"""The module-at-a-time drop-ins (deepinteract_amd/layers.py) on a ragged graph, against the oracle's
restatement of each module evaluated in float64 (tests/geot_cases.py: in_fp64).

tests/test_gpu_modules.py runs them on the tiny fixture only: uniform in-degree 20 and 960 edges, a
multiple of every block size. Here the graph is ragged37 with general edge features (37 nodes, 300
edges = one full 256-edge block plus 44; in-degrees 0 .. 40 with node 0 empty, self-loops and
duplicate edges), so k_attn_node sees a ragged in_ptr and an empty segment, and k_attn_edge and
di_conformation a partial block. Node and edge inputs are seeded random tensors; bounds as in
tests/test_gpu_modules.py (fp32 1e-4, bf16 1.6e-2 of the max-abs reference).
"""
import pytest
import torch

import geot_cases as C
from oracle import geot_oracle as O

pytestmark = pytest.mark.gpu
TOL = {"f32": 1e-4, "bf16": 1.6e-2}
P = "gnn_module.0.gt_block.0"


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def _np(t):
    return t.detach().float().cpu().numpy()


def _check(what, dtype, out, ref):
    err, row = C.check(_np(out).reshape(ref.shape[0], -1), ref.double().numpy().reshape(ref.shape[0], -1))
    print(f"ragged37 {what} {dtype}: {err:.3e} (worst row {row})")
    assert err <= TOL[dtype], (what, dtype, err, row)


@pytest.fixture(scope="module")
def case():
    from deepinteract_amd.graph import ResidueGraph
    it = C.ragged_item("ragged37", "general")
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    g.edata["src_nbr_e_ids"], g.edata["dst_nbr_e_ids"] = it["src_nbr"], it["dst_nbr"]
    assert g.num_edges() == 300 and not bool((it["dst"] == 0).any())  # node 0 has no in-edge
    og = {k: it[k] for k in ("num_nodes", "src", "dst", "src_nbr", "dst_nbr")}
    gen = torch.Generator().manual_seed(7)
    node = torch.randn(it["num_nodes"], 128, generator=gen)
    edge = torch.randn(g.num_edges(), 128, generator=gen)
    sd = C.state_dict(2)
    return g, og, node, edge, it["edge_f"], sd, C.to64(sd)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_init_edge_module(case, dtype):
    from deepinteract_amd.layers import InitEdgeModule
    g, og, _, _, G, sd, sd64 = case
    g.edata["f"] = G
    m = InitEdgeModule(dtype).load_reference_state_dict(_sub(sd, "gnn_module.0.init_edge_module."))
    _check("init_edge", dtype, m(g), C.in_fp64(O.init_edge, sd64, og, G.double()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_conformation_module(case, dtype):
    from deepinteract_amd.layers import ConformationModule
    g, og, _, edge, G, sd, sd64 = case
    g.edata["f"] = edge
    m = ConformationModule(dtype).load_reference_state_dict(_sub(sd, f"{P}.conformation_module."))
    ref = C.in_fp64(O.conformation, sd64, f"{P}.conformation_module", og, edge.double(), G.double())
    _check("conformation", dtype, m(g, G), ref)


@pytest.mark.parametrize("update_edge_feats", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mha_layer(case, dtype, update_edge_feats):
    from deepinteract_amd.layers import MultiHeadGeometricAttentionLayer
    g, og, node, edge, _, sd, sd64 = case
    m = MultiHeadGeometricAttentionLayer(128, 32, 4, False, update_edge_feats, dtype=dtype)
    m.load_reference_state_dict(_sub(sd, f"{P}.mha_module."))
    h, e = m(g, node, edge)
    rh, re = C.in_fp64(O.mha, sd64, f"{P}.mha_module", og, node.double(), edge.double(), update_edge_feats)
    assert h.shape == (node.shape[0], 4, 32)
    _check("mha node", dtype, h, rh)
    # the empty segment: node 0 aggregates nothing, 0 / (0 + 1e-6)
    assert not bool(rh[0].any()) and not bool(h[0].float().cpu().any()), h[0]
    if update_edge_feats:
        assert e.shape == (edge.shape[0], 4, 32)
        _check("mha edge", dtype, e, re)
    else:
        assert e is None


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_geometric_transformer_module(case, dtype, final):
    from deepinteract_amd.layers import FinalGeometricTransformerModule, GeometricTransformerModule
    g, og, node, edge, G, sd, sd64 = case
    li = 1 if final else 0
    g.ndata["f"], g.edata["f"] = node, edge
    cls = FinalGeometricTransformerModule if final else GeometricTransformerModule
    m = cls(dtype).load_reference_state_dict(_sub(sd, f"gnn_module.0.gt_block.{li}."))
    out = m(g, G)
    rn, re, _ = C.in_fp64(O.gt_layer, sd64, li, og, node.double(), edge.double(), G.double(), final)
    if final:
        _check("final gt node", dtype, out, rn)
    else:
        n, e = out
        _check("gt node", dtype, n, rn)
        _check("gt edge", dtype, e, re)
