"""disable_geometric_mode on the GPU: GeoTEngine's plain path (di_init_edge_plain, di_edge_layer_plain,
csrc/geot_plain.hip) against the float64 restatement tests/plain_cases.py::plain_forward64, which
tests/test_plain_host.py pins to the reference's own outputs, and LitGINI(disable_geometric_mode=True)
against the reference's fixture tests/golden/plain_tiny.npz.

Batches (tests/geot_cases.py): the ragged batch (2641 nodes, 2189 edges = 34 tiles of 64 + 13 rows;
in-degrees 0 .. 100, duplicate edges, chain offsets off every tile size) and the device-built kNN
batches of 21, 33, 420 and 820 edges (less than one tile, one wave's rows + 1, several tiles with a
tail). L = 1 pins the final layer's use of F0's hidden columns 0 / 1, L = 2 layer 0's edge output,
L = 3 a middle layer. Tolerances: geot_cases.TOL (fp32 1e-4, bf16 1.5e-2, max-abs error over max-abs
reference), the bounds of every other engine path.
"""
import numpy as np
import pytest
import torch

import geot_cases as C
import plain_cases as P
from gpu_common import close_elem, rel_elem, rel_max

pytestmark = pytest.mark.gpu

BATCHES = ["ragged_geo_ref"] + list(C.KNN_BATCHES)
N_MAX, E_MAX = 2641, 2189  # the ragged batch, the largest here


@pytest.fixture(scope="module")
def batches():
    from deepinteract_amd.builder import build_graph_batch
    from deepinteract_amd.graph import GraphBatch
    out = {"ragged_geo_ref": GraphBatch.from_arrays(C.ragged_batch_items("geo_ref"), "cuda")}
    for name, (sizes, k, edges) in C.KNN_BATCHES.items():
        chains, k, seeds = C.knn_chains(name)
        out[name] = gb = build_graph_batch(chains, k=k, nbr_seeds=seeds)
        assert gb.num_edges == edges
    assert (out["ragged_geo_ref"].num_nodes, out["ragged_geo_ref"].num_edges) == (N_MAX, E_MAX)
    return out


@pytest.fixture(scope="module")
def engines():
    """(dtype, L) -> plain engine, built on first use with a workspace slot beyond every batch."""
    from deepinteract_amd.engine import GeoTEngine
    made = {}

    def get(dtype, L):
        if (dtype, L) not in made:
            eng = GeoTEngine(P.state_dict(L), dtype, P.plain_cfg(L))
            assert eng.plain and eng.split_node and not eng.fold_attn
            eng.workspace(N_MAX + 64, E_MAX + 300)
            made[dtype, L] = eng
        return made[dtype, L]

    return get


def _poison(eng):
    (cap, bufs), n = eng._ws[0], 0
    assert cap == (N_MAX + 64, E_MAX + 300), cap
    for v in bufs.values():
        for t in (v if isinstance(v, list) else [v]):
            if t is not None:
                t.fill_(float("nan"))
                n += 1
    assert n >= 12


@pytest.mark.parametrize("split_node", [True, False], ids=["split_node", "fused_node"])
@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plain_engine_matches_plain_forward64(engines, batches, dtype, batch, L, split_node):
    eng, gb = engines(dtype, L), batches[batch]
    try:
        eng.split_node = split_node
        _poison(eng)
        events = {}
        h, e = eng.forward(gb, events=events)
        torch.cuda.synchronize()
    finally:
        eng.split_node = True
    assert "node_embed" in events and "init_edge" in events and "edge_layer_final" in events
    assert ("edge_layer" in events) == (L > 1) and ("node_aggr" in events) == split_node
    assert len(events.get("edge_layer", [])) == L - 1
    hT = eng.last_hT
    assert h.shape == (gb.num_nodes, 128) and e.shape == (gb.num_edges, 128) and hT.shape == (128, gb.num_nodes)
    assert eng._ws[0][0] == (N_MAX + 64, E_MAX + 300)  # the forward ran inside the poisoned slot
    for what, t in (("h", h), ("e", e), ("hT", hT)):
        bad = ~torch.isfinite(t.float())
        assert not bool(bad.any()), (what, "first non-finite (row, col)", bad.nonzero()[0].tolist(), int(bad.sum()))
    assert torch.equal(hT, h.t())
    hc, ec = h.float().cpu().numpy(), e.float().cpu().numpy()
    failures = []
    for g in range(len(gb.nodes_per_graph)):
        rn, re = P.plain_forward64(P.state_dict(L), C.oracle_item(gb, g), L, key=("gpu", batch, g))
        n0, n1, e0, e1 = gb.node_off[g], gb.node_off[g + 1], gb.edge_off[g], gb.edge_off[g + 1]
        (en, rown), (ee, rowe) = C.check(hc[n0:n1], rn), C.check(ec[e0:e1], re)
        print(f"plain {dtype} {batch} L={L} {'split' if split_node else 'fused'} chain {g}: node {en:.3e} edge {ee:.3e}")
        if not (en <= C.TOL[dtype] and ee <= C.TOL[dtype]):
            failures.append(f"chain {g}: node {en:.3e} at chain row {rown}, edge {ee:.3e} at chain row {rowe} of "
                            f"{e1 - e0} (batch row {e0 + rowe}: {(e0 + rowe) % 64} in its tile; Et = {gb.num_edges})")
    assert not failures, (C.TOL[dtype], failures)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_geo_ref_flag_is_ignored_and_runs_repeat(engines, batches, dtype):
    eng = engines(dtype, 2)
    for batch in ("ragged_geo_ref", "knn20_21_k20"):
        gb = batches[batch]
        assert gb.geo_ref
        h0, e0 = eng.forward(gb)
        h1, e1 = eng.forward(gb)
        h2, e2 = eng.forward(gb.with_geo_ref(False))
        torch.cuda.synchronize()
        assert torch.equal(h0, h1) and torch.equal(e0, e1), batch
        assert torch.equal(h0, h2) and torch.equal(e0, e2), batch


def test_fold_attn_is_refused(engines, batches):
    eng = engines("bf16", 2)
    try:
        eng.fold_attn = True
        with pytest.raises(ValueError, match="fold_attn"):
            eng.forward(batches["knn7_k3"])
    finally:
        eng.fold_attn = False


def _residue_graph(it):
    from deepinteract_amd.graph import ResidueGraph
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    g.ndata["f"], g.edata["f"] = it["node_f"], it["edge_f"]
    g.edata["src_nbr_e_ids"], g.edata["dst_nbr_e_ids"] = it["src_nbr"], it["dst_nbr"]
    return g.to("cuda")


def _fixture_model(dtype, **kw):
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    sd = seeded_state_dict(0, P.plain_cfg(2))
    return LitGINI(disable_geometric_mode=True, dtype=dtype, **kw).cuda().eval().load_reference_state_dict(sd)


def _fixture_step(model):
    z = P.fixture()
    g1, g2 = _residue_graph(P.fixture_item(z, "g1")), _residue_graph(P.fixture_item(z, "g2"))
    with torch.no_grad():
        logits, n1, e1, n2, e2 = model.shared_step(g1, g2, return_representations=True)
    assert model.engine.plain
    return z, logits, {"g1": (n1, e1), "g2": (n2, e2)}


def test_litgini_f32_against_the_reference_fixture():
    """The bars of tests/test_gpu_head_conv_f32.py::_check_model, and 1e-4 on the GeoT outputs."""
    from deepinteract_amd.head import contact_probs
    z, logits, reps = _fixture_step(_fixture_model("f32", precise_head=True))
    for tag, (n, e) in reps.items():
        en, ee = rel_max(n, z[f"{tag}_node_out"]), rel_max(e[z[f"{tag}_edge_rows"]], z[f"{tag}_edge_out"])
        print(f"plain LitGINI f32 {tag}: node {en:.3e} edge {ee:.3e}")
        assert e.shape[0] == z[f"{tag}_src"].shape[0]
        assert np.abs(e.astype(np.float64).sum(0) - z[f"{tag}_edge_out_colsum"]).max() <= 1e-4 * np.abs(e).sum(0).max()
        assert en < 1e-4 and ee < 1e-4, (tag, en, ee)
    lg = logits[0].detach().float().cpu().numpy()
    assert len(logits) == 1 and lg.shape == tuple(z["logits"].shape)
    ln, lc = rel_max(lg, z["logits"]), close_elem(lg, z["logits"])
    pe = rel_elem(contact_probs(logits[0]).detach().cpu().numpy(), z["probs"])
    print(f"plain LitGINI f32: logits normwise {ln:.3e}, allclose ratio {lc:.3f}, probabilities elementwise {pe:.3e}")
    assert ln < 1e-4 and lc <= 1.0 and pe < 1e-4


def test_litgini_bf16_geot_outputs_against_the_reference_fixture():
    z, _, reps = _fixture_step(_fixture_model("bf16"))
    for tag, (n, e) in reps.items():
        en, ee = rel_max(n, z[f"{tag}_node_out"]), rel_max(e[z[f"{tag}_edge_rows"]], z[f"{tag}_edge_out"])
        print(f"plain LitGINI bf16 {tag}: node {en:.3e} edge {ee:.3e}")
        assert en < 1.5e-2 and ee < 1.5e-2, (tag, en, ee)


def test_predict_batch_on_a_device_built_batch():
    """Two small complexes built on the device; the same model fed from_arrays copies of that batch."""
    from deepinteract_amd import synth
    from deepinteract_amd.builder import build_graph_batch
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    cfg = P.plain_cfg(2, num_interact_layers=1)
    model = LitGINI(disable_geometric_mode=True, num_interact_layers=1, dtype="f32").cuda().eval()
    model.load_reference_state_dict(seeded_state_dict(0, cfg))
    chains = [c for seed, (a, b) in ((3, (23, 31)), (4, (40, 22))) for c in synth.synthetic_complex(seed, a, b)]
    gb = build_graph_batch(chains)
    pairs = [(0, 1), (2, 3)]
    copy = GraphBatch.from_arrays([C.oracle_item(gb, g) for g in range(4)], "cuda")
    assert copy.num_edges == gb.num_edges == 20 * (23 + 31 + 40 + 22)
    with torch.no_grad():
        logits, probs = model.predict_batch(gb, pairs)
        h = model.engine.forward(gb)[0]
        logits2, probs2 = model.predict_batch(copy, pairs)
        h2 = model.engine.forward(copy)[0]
    torch.cuda.synchronize()
    assert [tuple(p.shape) for p in probs] == [(23, 31), (40, 22)]
    assert torch.equal(h, h2) and bool(torch.isfinite(h).all())
    for a, b in zip(logits + probs, logits2 + probs2):
        assert bool(torch.isfinite(a).all()) and rel_max(a.cpu().numpy(), b.cpu().numpy()) < 1e-5
