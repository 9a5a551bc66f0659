"""The attention clamps on the GPU: every place the HIP code restates

    score = clamp(K[src] * Q[dst] / sqrt(32), -5, 5) * P;  alpha = exp(clamp(sum_d score, -5, 5))

(graph_utils.py:29-32, :58-61) run with weights under which both clamps bind on 1 % .. 40 % of their
values in every layer (tests/geot_cases.py: SAT_FACTORS; tests/plain_cases.py for the plain mode;
tests/test_geot_cases_host.py and tests/test_plain_host.py hold the conditions on these inputs). No
other GPU test reaches a clamp: with the seeded weights no pre-clamp value exceeds 3.66.

Which test covers which restatement:
  csrc/geot_edge.hip, fp32 edge kernel     test_engine_path_matches_oracle64[f32-*], test_fixture_*[geo]
  csrc/geot_edge.hip, bf16 edge ring       test_engine_path_matches_oracle64[bf16-*]: "default" and
                                           "fused_node" take the z form of layer 0 (L >= 2, as built),
                                           "fold" the folded aggregation, the rest the plain F form
  csrc/modules.hip k_attn_edge             test_mha_layer
  csrc/geot_plain.hip                      test_plain_engine_matches_plain_forward64, test_fixture_*[plain]
Each wrong placement (a clamp dropped, the element clamp before the division) moves the float64
reference by more than twice the bound of every chain here (the host files assert it), so it fails
the chain's comparison; a bound of 5 changed on one side moves every saturated value on that side.

Bounds, per chain, L and output (geot_cases.sat_bounds): fp32 1e-4; bf16 1.5e-2 times
max(1, the reference's own bf16 sensitivity with these weights / with the seeded ones), computed here
on the CPU from the float64 reference alone and printed with -s.

The engine tests keep tests/test_gpu_geot_edge_shapes.py's structure (poisoned oversized workspace,
finite outputs, last_hT bit-equal, path assertions) and add: the float64 reference of the very batch
saw all four tails in every layer, and, where the final layer's alpha is a buffer of its own (every
path but "fold"), the device's alpha reaches both exp(-5) and exp(5) and nothing beyond.
"""
import math

import numpy as np
import pytest
import torch

import geot_cases as C
import plain_cases as P
from gpu_common import close_elem, rel_max
from oracle import geot_oracle as O

pytestmark = pytest.mark.gpu

# (batch, as built?)
FORMS = [("ragged_geo_ref", True), ("ragged_general", False), ("knn21_k20", True), ("knn21_k20", False)]
PLAIN_BATCHES = ["ragged_geo_ref"] + list(C.KNN_BATCHES)
N_MAX, E_MAX = 2641, 2189  # the ragged batch, the largest here
_refs = {}


@pytest.fixture(scope="module")
def batches():
    from deepinteract_amd.builder import build_graph_batch
    from deepinteract_amd.graph import GraphBatch
    out = {f"ragged_{f}": GraphBatch.from_arrays(C.ragged_batch_items(f), "cuda") for f in C.FEATS}
    assert out["ragged_geo_ref"].geo_ref and not out["ragged_general"].geo_ref
    for name, (sizes, k, edges) in C.KNN_BATCHES.items():
        chains, k, seeds = C.knn_chains(name)
        out[name] = gb = build_graph_batch(chains, k=k, nbr_seeds=seeds)
        assert gb.num_edges == edges and gb.geo_ref
    for gb in out.values():
        assert gb.num_nodes <= N_MAX and gb.num_edges <= E_MAX
    assert (out["ragged_geo_ref"].num_nodes, out["ragged_geo_ref"].num_edges) == (N_MAX, E_MAX)
    return out


def _engines(state_dict, cfg_of, check):
    made = {}

    def get(dtype, L):
        from deepinteract_amd.engine import GeoTEngine
        if (dtype, L) not in made:
            eng = GeoTEngine(state_dict(L), dtype, cfg_of(L))
            check(eng)
            eng.workspace(N_MAX + 64, E_MAX + 300)
            made[dtype, L] = eng
        return made[dtype, L]

    return get


@pytest.fixture(scope="module")
def engines():
    """(dtype, L) -> engine with the saturating weights and a workspace slot beyond every batch."""
    from deepinteract_amd.config import GeoTConfig

    def check(eng):
        assert {a: getattr(eng, a) for a in C.DEFAULTS} == C.DEFAULTS  # DI_INIT_Z=0 would hide the z path
    return _engines(C.saturating_state_dict, lambda L: GeoTConfig(num_gnn_layers=L), check)


@pytest.fixture(scope="module")
def plain_engines():
    def check(eng):
        assert eng.plain and eng.split_node and not eng.fold_attn
    return _engines(P.saturating_state_dict, P.plain_cfg, check)


def _poison(eng):
    (cap, bufs), n = eng._ws[0], 0
    assert cap == (N_MAX + 64, E_MAX + 300), cap
    for v in bufs.values():
        for t in (v if isinstance(v, list) else [v]):
            if t is not None:
                t.fill_(float("nan"))
                n += 1
    assert n >= 12


def _reference(mode, gb, batch, g, L):
    """(node, edge, tails, (bf16 node bound, bf16 edge bound)) of chain g of a device batch under the
    mode's saturating weights, in float64 on the CPU; one run per (mode, batch, chain, L)."""
    key = (mode, batch, g, L)
    if key not in _refs:
        item = C.oracle_item(gb, g)
        if mode == "geo":
            forward, sat_sd, seeded_sd = O.geot_forward, C.saturating_state_dict(L), C.state_dict(L)
        else:
            forward, sat_sd, seeded_sd = P.plain_forward, P.saturating_state_dict(L), P.state_dict(L, P.SAT_SEED)
        node, edge, tails = C.variant64(forward, sat_sd, item, L)
        sat = C.bf16_sensitivity(sat_sd, item, L, forward=forward)
        seeded = C.bf16_sensitivity(seeded_sd, item, L, forward=forward)
        bounds = C.sat_bounds("bf16", sat, seeded)
        print(f"saturated {mode} {batch} chain {g} L={L}: bf16 sensitivity saturating {sat[0]:.2e} / {sat[1]:.2e}, "
              f"seeded {seeded[0]:.2e} / {seeded[1]:.2e}, bf16 bounds node {bounds[0]:.2e} edge {bounds[1]:.2e}")
        for a in (node, edge):
            a.setflags(write=False)
        _refs[key] = (node, edge, tails, bounds)
    return _refs[key]


def _outputs_finite(eng, gb, h, e):
    hT = eng.last_hT
    assert h.shape == (gb.num_nodes, 128) and e.shape == (gb.num_edges, 128) and hT.shape == (128, gb.num_nodes)
    assert eng._ws[0][0] == (N_MAX + 64, E_MAX + 300)  # the forward ran inside the poisoned slot
    for what, t in (("h", h), ("e", e), ("hT", hT)):
        bad = ~torch.isfinite(t.float())
        assert not bool(bad.any()), (what, "first non-finite (row, col)", bad.nonzero()[0].tolist(), int(bad.sum()))
    assert torch.equal(hT, h.t())


def _alpha_reaches_both_bounds(eng, gb):
    """The final layer's alpha = exp(clamp(head sum)): both bounds reached, nothing beyond. 1e-5: the
    hardware exponential is a few ulp from exp(+-5)."""
    alpha = eng._ws[0][1]["alpha"][:gb.num_edges].double().cpu().numpy()
    assert np.isfinite(alpha).all()
    lo, hi = math.exp(-5.0), math.exp(5.0)
    assert abs(alpha.min() / lo - 1) <= 1e-5 and abs(alpha.max() / hi - 1) <= 1e-5, (alpha.min() / lo, alpha.max() / hi)


def _compare(mode, tag, dtype, gb, batch, L, h, e, tile):
    hc, ec = h.float().cpu().numpy(), e.float().cpu().numpy()
    in_ptr = gb.in_ptr.cpu()
    failures = []
    for g in range(len(gb.nodes_per_graph)):
        rn, re, tails, bf16_bounds = _reference(mode, gb, batch, g, L)
        # the reference of these very numbers met every clamp in every layer
        assert len(tails) == L and all(t[k] > 0 for t in tails for k in C.TAILS), tails
        bn, be = C.sat_bounds("f32") if dtype == "f32" else bf16_bounds
        n0, n1, e0, e1 = gb.node_off[g], gb.node_off[g + 1], gb.edge_off[g], gb.edge_off[g + 1]
        (en, rown), (ee, rowe) = C.check(hc[n0:n1], rn), C.check(ec[e0:e1], re)
        print(f"geot_saturated {tag} L={L} chain {g}: node {en:.3e} (bound {bn:.2e}) edge {ee:.3e} (bound {be:.2e})")
        if not (en <= bn and ee <= be):
            v = n0 + rown
            failures.append(f"chain {g}: node {en:.3e} > {bn:.2e} at chain row {rown} (in-degree {int(in_ptr[v + 1] - in_ptr[v])}), "
                            f"edge {ee:.3e} > {be:.2e} at chain row {rowe} of {e1 - e0} (batch row {e0 + rowe}: "
                            f"{(e0 + rowe) % tile} in its {tile}-row tile; Et = {gb.num_edges})")
    assert not failures, failures


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("batch,as_built", FORMS, ids=[f"{b}-{'as_built' if a else 'general_path'}" for b, a in FORMS])
@pytest.mark.parametrize("dtype,path", list(C.PATHS), ids=[f"{d}-{p}" for d, p in C.PATHS])
def test_engine_path_matches_oracle64(engines, batches, dtype, path, batch, as_built, L):
    from deepinteract_amd.engine import uses_z_init
    eng = engines(dtype, L)
    gb = batches[batch] if as_built else batches[batch].with_geo_ref(False)
    assert gb.geo_ref == as_built
    try:
        for attr, val in C.PATHS[dtype, path].items():
            setattr(eng, attr, val)
        # what the path table means, stated apart from the engine's own dispatch
        want_z = dtype == "bf16" and path in ("default", "fused_node") and as_built and L >= 2
        want_embed_launch = path.startswith("unfused") or not as_built
        want_split = path not in ("fused_node", "fold")
        assert uses_z_init(eng, gb) == want_z
        _poison(eng)
        before, events = eng.z_forwards, {}
        h, e = eng.forward(gb, events=events)
        torch.cuda.synchronize()
        assert eng.z_forwards - before == int(want_z)
        assert ("node_embed" in events) == want_embed_launch, sorted(events)
        assert ("node_aggr" in events) == want_split, sorted(events)
        assert "init_edge" in events and "edge_layer_final" in events and ("edge_layer" in events) == (L > 1)
        _outputs_finite(eng, gb, h, e)
        if path != "fold":  # the folded aggregation keeps alpha in registers
            _alpha_reaches_both_bounds(eng, gb)
    finally:
        for attr, val in C.DEFAULTS.items():
            setattr(eng, attr, val)
    _compare("geo", f"{dtype} {path} {batch} {'as_built' if as_built else 'general_path'}", dtype, gb, batch, L, h, e, 256)


@pytest.mark.parametrize("split_node", [True, False], ids=["split_node", "fused_node"])
@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("batch", PLAIN_BATCHES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plain_engine_matches_plain_forward64(plain_engines, batches, dtype, batch, L, split_node):
    eng, gb = plain_engines(dtype, L), batches[batch]
    try:
        eng.split_node = split_node
        _poison(eng)
        events = {}
        h, e = eng.forward(gb, events=events)
        torch.cuda.synchronize()
        assert "node_embed" in events and "init_edge" in events and "edge_layer_final" in events
        assert ("edge_layer" in events) == (L > 1) and ("node_aggr" in events) == split_node
        _outputs_finite(eng, gb, h, e)
        if batch not in C.TINY_KNN:  # 84 / 132 head sums need not reach both bounds in the final layer
            _alpha_reaches_both_bounds(eng, gb)
    finally:
        eng.split_node = True
    _compare("plain", f"plain {dtype} {batch} {'split' if split_node else 'fused'}", dtype, gb, batch, L, h, e, 64)


# ---- the module-at-a-time drop-in (csrc/modules.hip: k_attn_edge)
MHA_TOL = {"f32": 1e-4, "bf16": 1.6e-2}  # tests/test_gpu_modules_ragged.py's
MHA = "gnn_module.0.gt_block.0.mha_module."


@pytest.fixture(scope="module")
def mha_case():
    """ragged37 / general and what layer 0 of the saturating two-layer model feeds its mha_module there
    (the normalised node embedding and conformation output, from the float32 oracle): the activations
    block 0's factors are calibrated for. Seeded N(0, 1) inputs, as tests/test_gpu_modules_ragged.py
    uses, saturate 90 % of the head sums under these weights, and the float64 reference itself then
    moves by 4.1e-2 under bf16 rounding."""
    from deepinteract_amd.graph import ResidueGraph
    it = C.ragged_item("ragged37", "general")
    g = ResidueGraph(it["src"], it["dst"], it["num_nodes"])
    og = {k: it[k] for k in ("num_nodes", "src", "dst")}
    sd, seen, prev = C.saturating_state_dict(2), {}, O.mha

    def grab(sd_, p, g_, node, edge, update_edge_feats):
        seen.setdefault(p, (node.clone(), edge.clone()))
        return prev(sd_, p, g_, node, edge, update_edge_feats)

    O.mha = grab
    try:
        C.oracle32(sd, it, 2)
    finally:
        O.mha = prev
    node, edge = seen[MHA[:-1]]
    assert node.shape == (37, 128) and edge.shape == (300, 128) and node.dtype == torch.float32
    return g, og, node, edge, sd, C.to64(sd)


@pytest.mark.parametrize("update_edge_feats", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mha_layer(mha_case, dtype, update_edge_feats):
    """Block 0's scaled mha_module weights against geot_cases.mha_variant at the reference's setting
    (equal to oracle.mha, asserted) in float64, which must have seen all four tails and which every
    wrong clamp placement must miss by more than twice the bound."""
    from deepinteract_amd.layers import MultiHeadGeometricAttentionLayer
    g, og, node, edge, sd, sd64 = mha_case
    args = (sd64, MHA[:-1], og, node.double(), edge.double(), update_edge_feats)
    tails = []
    rh, re = C.in_fp64(C.mha_variant(tails=tails), *args)
    oh, oe = C.in_fp64(O.mha, *args)
    assert torch.equal(rh, oh) and (oe is None or torch.equal(re, oe))
    (t,) = tails
    print(f"mha_layer ragged37 tails: {dict(zip(C.TAILS, C.tail_fractions(t)))}")
    assert all(t[k] > 0 for k in C.TAILS), t
    for name, switches in C.MUTANTS.items():
        mh, me = C.in_fp64(C.mha_variant(**switches), *args)
        errs = [rel_max(mh.numpy(), rh.numpy())] + ([rel_max(me.numpy(), re.numpy())] if update_edge_feats else [])
        assert max(errs) > 2 * MHA_TOL["bf16"], (name, errs)
    m = MultiHeadGeometricAttentionLayer(128, 32, 4, False, update_edge_feats, dtype=dtype)
    m.load_reference_state_dict({k[len(MHA):]: v for k, v in sd.items() if k.startswith(MHA)})
    h, e = m(g, node, edge)
    assert h.shape == (node.shape[0], 4, 32)
    outs = [("node", h, rh)] + ([("edge", e, re)] if update_edge_feats else [])
    assert update_edge_feats or e is None
    for what, out, ref in outs:
        err, row = C.check(out.detach().float().cpu().numpy().reshape(ref.shape[0], -1), ref.numpy().reshape(ref.shape[0], -1))
        print(f"mha_layer saturated {what} {dtype} update_edge_feats={update_edge_feats}: {err:.3e} (worst row {row})")
        assert err <= MHA_TOL[dtype], (what, dtype, err, row)
    assert not bool(rh[0].any()) and not bool(h[0].float().cpu().any())  # node 0 has no in-edge


# ---- the reference's own outputs under saturating weights (tests/golden/sat_tiny.npz)
def _fixture_weights(mode, with_head):
    from deepinteract_amd.weights import seeded_state_dict
    if mode == "geo":
        return C.scale_attention(seeded_state_dict(0, with_head=with_head), {li: C.SAT_FACTORS[li] for li in range(2)})
    return C.scale_attention(seeded_state_dict(P.SAT_SEED, P.plain_cfg(2), with_head=with_head), P.block_factors(2))


@pytest.mark.parametrize("mode", ["geo", "plain"])
def test_fixture_f32_engine(mode):
    """The bounds of tests/test_gpu_parity.py / tests/test_gpu_plain.py on tiny / plain_tiny: 1e-4."""
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.engine import GeoTEngine
    from deepinteract_amd.graph import GraphBatch
    z = np.load(C.SAT_GOLDEN)
    gb = GraphBatch.from_arrays([C.fixture_item(z, "g1"), C.fixture_item(z, "g2")], "cuda")
    eng = GeoTEngine(_fixture_weights(mode, False), "f32", P.plain_cfg(2) if mode == "plain" else GeoTConfig())
    assert eng.plain == (mode == "plain")
    h, e = eng.forward(gb)
    torch.cuda.synchronize()
    h, e = h.cpu().numpy(), e.cpu().numpy()
    for g, tag in enumerate(("g1", "g2")):
        n0, n1, e0, e1 = gb.node_off[g], gb.node_off[g + 1], gb.edge_off[g], gb.edge_off[g + 1]
        eg = e[e0:e1]
        en = rel_max(h[n0:n1], z[f"{mode}_{tag}_node_out"])
        ee = rel_max(eg[z[f"{mode}_{tag}_edge_rows"]], z[f"{mode}_{tag}_edge_out"])
        print(f"saturated fixture {mode} f32 engine {tag}: node {en:.3e} edge {ee:.3e}")
        assert np.abs(eg.astype(np.float64).sum(0) - z[f"{mode}_{tag}_edge_out_colsum"]).max() <= 1e-4 * np.abs(eg).sum(0).max()
        assert en < 1e-4 and ee < 1e-4, (tag, en, ee)


@pytest.mark.parametrize("mode", ["geo", "plain"])
def test_fixture_f32_logits(mode):
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.modules import LitGINI
    z = np.load(C.SAT_GOLDEN)
    model = LitGINI(dtype="f32", precise_head=True, disable_geometric_mode=mode == "plain").cuda().eval()
    model.load_reference_state_dict(_fixture_weights(mode, True))
    gb = GraphBatch.from_arrays([C.fixture_item(z, "g1"), C.fixture_item(z, "g2")], "cuda")
    with torch.no_grad():
        logits, _ = model.predict_batch(gb, [(0, 1)])
    torch.cuda.synchronize()
    lg, ref = logits[0].cpu().numpy(), z[f"{mode}_logits"]
    assert lg.shape == ref.shape
    ln, lc = rel_max(lg, ref), close_elem(lg, ref)
    print(f"saturated fixture {mode} f32 logits: normwise {ln:.3e}, allclose ratio {lc:.3f}")
    assert ln < 1e-4 and lc <= 1.0
