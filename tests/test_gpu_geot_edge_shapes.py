"""Every GeoTEngine path against the oracle in float64 (tests/geot_cases.py: oracle64) on ragged and
tail shapes, at one, two and three layers.

Batches:
  * the ragged batch [ragged37, sparse2304, ragged300] (2641 nodes, 2189 edges; in-degrees 0 .. 100,
    self-loops, duplicate edges, node_pos up to 2303, a middle chain that puts the third chain's node
    and edge offsets off every tile size), reference-featurised and general-featurised;
  * device-built kNN batches of 21, 33, 420 and 820 edges (tests/test_gpu_wide_rows.py's, plus 420).
Each runs as built and with_geo_ref(False) (the general kernels on the same numbers); the general-
featurised ragged batch has only the latter.

Paths (PATHS): attribute settings of one engine per (dtype, L), restored after each test. L = 1 pins
InitEdge's output and the final layer alone, L = 2 layer 0's edge output, L = 3 a middle layer.

Every (path, batch, L):
  1. the path that ran is the one meant: z_forwards rises by uses_z_init, which equals what the path
     table says; the timed launches contain node_embed iff the embedding was a launch of its own and
     node_aggr iff the split node layer ran;
  2. the workspace slot is larger than every batch (64 node rows, 300 edge rows beyond the largest)
     and every buffer of it is NaN before the forward; h, e and last_hT are finite afterwards, so no
     valid output depends on a row beyond the batch or on a buffer the path does not write;
  3. every chain's h[n0:n1] and e[e0:e1] against that chain's own oracle64 run: fp32 <= 1e-4, bf16 <=
     1.5e-2 (max-abs error / max-abs reference; BASELINE.json north_star, tests/test_gpu_parity.py).
     No reference row is below 0.1 of its tensor's maximum and the checker catches a copied or zeroed
     tail row and a shifted chain (tests/test_geot_cases_host.py);
  4. last_hT equals h transposed, bit for bit.
Measured errors are printed with -s (DESIGN.md section 2 holds the largest per path family and batch).
"""
import pytest
import torch

import geot_cases as C

pytestmark = pytest.mark.gpu

PATHS, DEFAULTS = C.PATHS, C.DEFAULTS  # the path table, shared with tests/test_gpu_geot_saturated.py
# (batch, as built?): the general-featurised ragged batch is the general path as built
FORMS = [("ragged_geo_ref", True), ("ragged_geo_ref", False), ("ragged_general", False)] + \
        [(name, form) for name in C.KNN_BATCHES for form in (True, False)]
N_MAX, E_MAX = 2641, 2189  # the ragged batch, the largest here


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
    assert int(out["ragged_geo_ref"].node_pos.max()) == 2303
    return out


@pytest.fixture(scope="module")
def engines():
    """(dtype, L) -> engine, built on first use with a workspace slot beyond every batch."""
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.engine import GeoTEngine
    made = {}

    def get(dtype, L):
        if (dtype, L) not in made:
            eng = GeoTEngine(C.state_dict(L), dtype, GeoTConfig(num_gnn_layers=L))
            assert {a: getattr(eng, a) for a in DEFAULTS} == DEFAULTS  # DI_INIT_Z=0 would hide the z path
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


def _reference(batches, batch, g, L):
    # the device-built batch's own numbers (with_geo_ref(False) shares them): one run per chain and L
    return C.oracle64(C.state_dict(L), C.oracle_item(batches[batch], g), L, key=("gpu", batch, g))


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("batch,as_built", FORMS, ids=[f"{b}-{'as_built' if a else 'general_path'}" for b, a in FORMS])
@pytest.mark.parametrize("dtype,path", list(PATHS), ids=[f"{d}-{p}" for d, p in PATHS])
def test_engine_path_matches_oracle64(engines, batches, dtype, path, batch, as_built, L):
    from deepinteract_amd.engine import uses_z_init
    eng = engines(dtype, L)
    gb = batches[batch] if as_built else batches[batch].with_geo_ref(False)
    assert gb.geo_ref == as_built
    try:
        for attr, val in PATHS[dtype, path].items():
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
        hT = eng.last_hT
        assert h.shape == (gb.num_nodes, 128) and e.shape == (gb.num_edges, 128) and hT.shape == (128, gb.num_nodes)
        assert eng._ws[0][0] == (N_MAX + 64, E_MAX + 300)  # the forward ran inside the poisoned slot
        for what, t in (("h", h), ("e", e), ("hT", hT)):
            bad = ~torch.isfinite(t.float())
            assert not bool(bad.any()), (what, "first non-finite (row, col)", bad.nonzero()[0].tolist(), int(bad.sum()))
        assert torch.equal(hT, h.t())
    finally:
        for attr, val in DEFAULTS.items():
            setattr(eng, attr, val)
    hc, ec = h.float().cpu().numpy(), e.float().cpu().numpy()
    in_ptr = gb.in_ptr.cpu()
    failures = []
    for g in range(len(gb.nodes_per_graph)):
        rn, re = _reference(batches, batch, g, L)
        n0, n1, e0, e1 = gb.node_off[g], gb.node_off[g + 1], gb.edge_off[g], gb.edge_off[g + 1]
        (en, rown), (ee, rowe) = C.check(hc[n0:n1], rn), C.check(ec[e0:e1], re)
        print(f"geot_edge_shapes {dtype} {path} {batch} {'as_built' if as_built else 'general_path'} L={L} chain {g}: "
              f"node {en:.3e} edge {ee:.3e}")
        if not (en <= C.TOL[dtype] and ee <= C.TOL[dtype]):
            # name the rows: node row, its in-degree; edge row, its place in the batch's 32- and 256-row tiles
            v = n0 + rown
            failures.append(f"chain {g}: node {en:.3e} at chain row {rown} (in-degree {int(in_ptr[v + 1] - in_ptr[v])}), "
                            f"edge {ee:.3e} at chain row {rowe} of {e1 - e0} (batch row {e0 + rowe}: "
                            f"{(e0 + rowe) % 32} in its wave, {(e0 + rowe) % 256} in its tile; Et = {gb.num_edges})")
    assert not failures, (C.TOL[dtype], failures)
