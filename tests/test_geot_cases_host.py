"""What the fp64 comparisons of tests/test_gpu_geot_edge_shapes.py rest on, checked without a GPU
(tests/geot_cases.py; kNN chains featurised on the CPU by oracle.build_graph):

* the cases have the shapes they are there for (edge counts off the tile sizes, the in-degrees, the
  last positional row);
* oracle64 (the oracle run in float64) agrees with the fp32 oracle within 1e-5 on every chain at
  L = 1, 2, 3 -- reference against reference, measured <= 1.3e-6, so the bound only guards the dtype
  switch;
* no row of any reference output is small: max|row| >= 0.1 max|tensor|, so a dropped, zeroed or
  swapped row costs far more than either GPU bound (1e-4, 1.5e-2). A condition on the seeds, not a
  measurement: if a seed change breaks it, change the seed;
* the checker, applied per chain as the GPU file applies it, reports more than the bf16 bound for
  the failures a tile kernel makes: the last edge row a copy of the row before it (a clamped tail
  lane stored), the last edge row zero (a tail row not stored), the last chain's node rows shifted by
  one (a wrong node offset for the third chain of the ragged batch).

And what tests/test_gpu_geot_saturated.py rests on: the same chains under geot_cases'
saturating weights. These are conditions on the inputs; if a case breaks one, the factors or a seed
change, never the condition:
* geot_cases.mha_variant at the reference's setting reproduces oracle64 bit for bit;
* in every layer each of the four clamp tails (element / head sum, below -5 / above 5) holds 1 % to
  40 % of its values, so every clamp binds without the head sums turning into a step function (the two
  tiny kNN chains, 84 and 132 head sums: at least one value per tail);
* oracle32 stays within 1e-5 of oracle64 (measured <= 2.2e-6), and no reference row is small;
* each wrong clamp placement (geot_cases.MUTANTS) misses oracle64, on the node or the edge output,
  by more than twice the bound the GPU file applies to that chain and L: fp32 1e-4, bf16 1.5e-2 times
  the ratio by which the reference moves more under bf16 rounding with the saturating weights than
  with the seeded ones (the two tiny kNN chains: fp32 only).
"""
import numpy as np
import pytest
import torch

import geot_cases as C
from oracle import geot_oracle as O

CASES = C.host_cases()
CHAINS = [(name, g) for name, items in CASES.items() for g in range(len(items))]


def _ref(name, g, L):
    return C.oracle64(C.state_dict(L), CASES[name][g], L, key=("host", name, g))


def test_ragged_shapes():
    for feats in C.FEATS:
        a, b, c = C.ragged_batch_items(feats)
        deg = [torch.bincount(it["dst"], minlength=it["num_nodes"]) for it in (a, b, c)]
        assert deg[0][:10].tolist() == [0, 1, 8, 9, 17, 40, 31, 32, 33, 16] and int(deg[0][10:].max()) <= 8
        assert deg[2][:6].tolist() == [0, 1, 16, 17, 40, 100] and int(deg[2][6:].max()) <= 12
        assert b["num_nodes"] == 2304 and {v: int(d) for v, d in enumerate(deg[1]) if d} == C.SPARSE_DEG
        assert int(b["src"][0]) == int(b["src"][-1]) == 2303 and int(b["dst"][-1]) == 2303
        counts = [it["src"].numel() for it in (a, b, c)]
        assert counts == [300, 42, 1847]
        # every chain and the batch off the 32-edge wave and the 256-edge tile; the third chain's
        # node and edge offsets off every tile size
        for e in counts + [sum(counts)]:
            assert e % 32 != 0 and e % 256 != 0, e
        n_off, e_off = a["num_nodes"] + b["num_nodes"], counts[0] + counts[1]
        assert all(n_off % t and e_off % t for t in (16, 32, 64, 256)), (n_off, e_off)
        for it in (a, b, c):
            E = it["src"].numel()
            assert bool((it["dst"][1:] >= it["dst"][:-1]).all())
            assert 0 <= int(it["src"].min()) and int(it["src"].max()) < it["num_nodes"]
            assert it["src_nbr"].shape == it["dst_nbr"].shape == (E, 2)
            assert 0 <= int(min(it["src_nbr"].min(), it["dst_nbr"].min()))
            assert int(max(it["src_nbr"].max(), it["dst_nbr"].max())) < E
            assert it["node_f"].shape == (it["num_nodes"], 113) and it["edge_f"].shape == (E, 28)
        assert bool((a["src"] == a["dst"]).any()) and bool((c["src"] == c["dst"]).any())  # self-loops
        pairs = c["src"] * 300 + c["dst"]
        assert pairs.unique().numel() < pairs.numel()  # duplicate edges


def test_featurisations():
    from deepinteract_amd.graph import edge_feats_geo_ref
    for name in C.RAGGED_BATCH:
        ref, gen = C.ragged_item(name, "geo_ref"), C.ragged_item(name, "general")
        assert edge_feats_geo_ref(ref["edge_f"]) and not edge_feats_geo_ref(gen["edge_f"])
        assert torch.equal(ref["edge_f"][:, :20], gen["edge_f"][:, :20]) and torch.equal(ref["src"], gen["src"])
        assert torch.allclose(gen["edge_f"][:, 23:27].norm(dim=1), torch.ones(gen["edge_f"].shape[0]))
    for name, (sizes, k, edges) in C.KNN_BATCHES.items():
        assert sum(it["src"].numel() for it in CASES[name]) == edges == sum(sizes) * k
        assert all(edge_feats_geo_ref(it["edge_f"]) for it in CASES[name])


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name,g", CHAINS)
def test_oracle64_matches_oracle32(name, g, L):
    n64, e64 = _ref(name, g, L)
    n32, e32 = C.oracle32(C.state_dict(L), CASES[name][g], L)
    assert n32.dtype == np.float32 and n64.dtype == np.float64
    en, _ = C.check(n32, n64)
    ee, _ = C.check(e32, e64)
    print(f"{name} chain {g} L={L}: oracle32 vs oracle64 node {en:.2e} edge {ee:.2e}")
    assert max(en, ee) <= 1e-5, (en, ee)


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name,g", CHAINS)
def test_no_small_reference_row(name, g, L):
    for what, ref in zip(("node", "edge"), _ref(name, g, L)):
        ratio = np.abs(ref).max(axis=1) / np.abs(ref).max()
        print(f"{name} chain {g} L={L} {what}: smallest row max / tensor max {ratio.min():.3f}")
        assert ratio.min() >= 0.1, (what, int(ratio.argmin()), float(ratio.min()))


def _per_chain_worst(name, L, node, edge):
    """The GPU file's comparison: each chain's slice of the batch outputs against its own reference."""
    worst, n0, e0 = 0.0, 0, 0
    for g in range(len(CASES[name])):
        rn, re = _ref(name, g, L)
        worst = max(worst, C.check(node[n0:n0 + len(rn)], rn)[0], C.check(edge[e0:e0 + len(re)], re)[0])
        n0, e0 = n0 + len(rn), e0 + len(re)
    return worst


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name", list(CASES))
def test_checker_catches_row_mutations(name, L):
    refs = [_ref(name, g, L) for g in range(len(CASES[name]))]
    node, edge = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    assert len(edge) >= 2
    assert _per_chain_worst(name, L, node, edge) == 0.0
    last = len(node) - len(refs[-1][0])  # first node row of the last chain (the third of the ragged batch)
    mutants = {"last edge row = the row before": (node, np.concatenate([edge[:-1], edge[-2:-1]])),
               "last edge row zero": (node, np.concatenate([edge[:-1], np.zeros_like(edge[-1:])])),
               "last chain's node rows shifted by one": (np.concatenate([node[:last], np.roll(node[last:], 1, 0)]), edge)}
    for what, (n, e) in mutants.items():
        err = _per_chain_worst(name, L, n, e)
        print(f"{name} L={L} {what}: {err:.3f}")
        assert err > C.TOL["bf16"], (what, err)


def test_check_names_the_row():
    ref = np.ones((5, 4))
    got = ref.copy()
    got[3, 2] += 0.5
    assert C.check(got, ref) == (0.5, 3)
    got[1, 0] = np.nan
    err, row = C.check(got, ref)
    assert np.isnan(err) and row == 1
    with pytest.raises(AssertionError, match="worst row 1 of 5"):
        C.check(got, ref, 1.0)
    with pytest.raises(AssertionError, match="worst row 3 of 5"):
        C.check(np.nan_to_num(got, nan=1.0), ref, 1e-4)


_sat = {}


def _sat_ref(name, g, L):
    """(node, edge, tails) of the saturating case, with the restatement checked against oracle64."""
    if (name, g, L) not in _sat:
        sd, item = C.saturating_state_dict(L), CASES[name][g]
        node, edge, tails = C.variant64(O.geot_forward, sd, item, L)
        rn, re = C.oracle64(sd, item, L, key=("host-sat", name, g))
        assert np.array_equal(node, rn) and np.array_equal(edge, re)  # the reference setting IS oracle.mha
        _sat[name, g, L] = (rn, re, tails)
    return _sat[name, g, L]


def test_saturating_state_dict_scales_only_the_attention_inputs():
    for L in C.LAYERS:
        base, sat = C.state_dict(L), C.saturating_state_dict(L)
        assert list(base) == list(sat)
        changed = {k for k in base if not torch.equal(base[k], sat[k])}
        want = {f"gnn_module.0.gt_block.{li}.mha_module.{m}.weight" for li in range(L) for m in ("Q", "K", "edge_feats_projection")}
        assert changed == want
        for li in range(L):
            p = f"gnn_module.0.gt_block.{li}.mha_module"
            assert torch.equal(sat[f"{p}.K.weight"], base[f"{p}.K.weight"] * C.SAT_FACTORS[li][0])
            assert torch.equal(sat[f"{p}.edge_feats_projection.weight"], base[f"{p}.edge_feats_projection.weight"] * C.SAT_FACTORS[li][1])


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name,g", CHAINS)
def test_saturating_tails(name, g, L):
    tails = _sat_ref(name, g, L)[2]
    for t in tails:
        print(f"{name} chain {g} L={L} {t['layer']}: " + ", ".join(f"{k} {f:.3f}" for k, f in zip(C.TAILS, C.tail_fractions(t))))
    C.check_tail_window(name, tails)


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name,g", CHAINS)
def test_saturating_oracle32_and_rows(name, g, L):
    n64, e64, _ = _sat_ref(name, g, L)
    n32, e32 = C.oracle32(C.saturating_state_dict(L), CASES[name][g], L)
    en, ee = C.check(n32, n64)[0], C.check(e32, e64)[0]
    print(f"saturating {name} chain {g} L={L}: oracle32 vs oracle64 node {en:.2e} edge {ee:.2e}")
    assert max(en, ee) <= 1e-5, (en, ee)
    for what, ref in (("node", n64), ("edge", e64)):
        ratio = np.abs(ref).max(axis=1) / np.abs(ref).max()
        assert ratio.min() >= 0.1, (what, int(ratio.argmin()), float(ratio.min()))


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name,g", CHAINS)
def test_saturating_mutants_are_decisive(name, g, L):
    n64, e64, _ = _sat_ref(name, g, L)
    item = CASES[name][g]
    sat = C.bf16_sensitivity(C.saturating_state_dict(L), item, L, key=("host-sat", name, g))
    seeded = C.bf16_sensitivity(C.state_dict(L), item, L, key=("host", name, g))
    bounds = C.sat_bounds("bf16", sat, seeded)
    errors = C.mutant_errors(O.geot_forward, C.saturating_state_dict(L), item, L, (n64, e64))
    print(f"saturating {name} chain {g} L={L}: bf16 sensitivity saturating {sat[0]:.2e} / {sat[1]:.2e}, seeded "
          f"{seeded[0]:.2e} / {seeded[1]:.2e}, bf16 bounds {bounds[0]:.2e} / {bounds[1]:.2e}; mutants "
          + ", ".join(f"{m} {a:.2e} / {b:.2e}" for m, (a, b) in errors.items()))
    C.check_decisive(name, errors, bounds)
