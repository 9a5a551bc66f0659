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
"""
import numpy as np
import pytest
import torch

import geot_cases as C

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
