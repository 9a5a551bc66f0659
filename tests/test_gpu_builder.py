"""The on-device graph builder (csrc/graph_builder.hip, sequenced by deepinteract_amd/builder.py)
against references computed at test time, at the shapes the fixtures do not reach: k = 3/20/30,
chains of n = k, k + 1 ... 4096 residues, 16-chain and mixed-length launches.

Two kinds of reference, one per kind of claim:

* exact claims (kNN tie order on lattice points, topology, torch-seeded neighbour ids): the CPU
  torch ops the reference itself calls (`torch.topk`, `torch.randperm`) through `oracle.knn` /
  `oracle.build_graph`, on inputs whose answer does not depend on the host;
* tolerance claims (kNN on real-valued chains, features): a float64 evaluation of the oracle's own
  formulas fed with the device's upstream outputs (its knn_idx / knn_d2), so each stage is judged
  alone. The fp32 oracle on the GPU host is never the yardstick for a tolerance: it is only
  required to sit within half of each bound of the float64 values on the chosen inputs.

Feature bounds are the project's own (test_gpu_parity.py::test_featuriser_matches_reference):
node features and edge columns 0-26 <= 2e-4 abs, amide-angle column 27 <= 2e-3 abs.

Measured on MI355X: see DESIGN.md section 2 ("Device builder at edge shapes").
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NODE_TOL = 2e-4
EDGE_TOL = 2e-4
AMIDE_TOL = 2e-3
GEO_REF = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


# ------------------------------------------------------------------------------- device builds
def _device_build(chains, k, node_count_limit=4096, nbr_seeds=None):
    """One build_graph_batch call; every output copied to the host (int64 / float32 tensors)."""
    from deepinteract_amd.builder import build_graph_batch
    gb, aux = build_graph_batch(chains, k=k, seed=1, device="cuda", return_aux=True,
                                node_count_limit=node_count_limit, nbr_seeds=nbr_seeds)
    torch.cuda.synchronize()
    out = {"k": k, "sizes": list(gb.nodes_per_graph), "node_off": list(gb.node_off), "edge_off": list(gb.edge_off)}
    for name in ("src", "dst", "nbr", "in_ptr", "node_pos"):
        out[name] = getattr(gb, name).cpu().long()
    out["node_f"], out["edge_f"] = gb.node_f.cpu(), gb.edge_f.cpu()
    out["knn_idx"], out["knn_d2"] = aux["knn_idx"].cpu().long(), aux["knn_d2"].cpu()
    return out


# name -> (k, chain lengths); n = k selects only k values, n = k + 1 is the first full k + 1 selection,
# 4096 is KNN_MAX_N (96 KiB of LDS), 16 x 1000 is the bench pool's shape, 255/256/257 nodes straddle
# k_knn_graph's launch boundary (grid Nt / 256 + 1; thread v == Nt writes the last in_ptr)
#
# The synth seeds are the first of base + g, base + g + 100, ... at which the fp32 oracle formulas
# stay within the condition of _feature_chain_check with margin (node <= 0.7e-4, amide <= 0.7e-3,
# searched on the CPU with the host's kNN; the node columns depend on the backbone alone).
BATCHES = {
    "k20_edges": (20, [20, 21, 64, 333, 1000], [3000, 3001, 3002, 3003, 3004]),
    "k30_4000": (30, [30, 97, 4000], [5000, 5001, 5402]),
    "k20_4096": (20, [4096, 20], [2100, 2001]),
    "k3": (3, [40, 7], [4000, 4001]),
    "k20_16x1000": (20, [1000] * 16, [1000, 1101, 1002, 1003, 1004, 1005, 1006, 1107, 1308, 1209, 1010, 1011,
                                     1012, 1013, 1014, 1015]),
}
TOPOLOGY_ONLY = {
    "nt255": (20, [235, 20], [6000, 6001]),
    "nt256": (20, [236, 20], [6100, 6101]),
    "nt257": (20, [237, 20], [6200, 6201]),
}
_CACHE = {}


def _batch(name):
    """The chains of a named batch and their device build, made once per session and left unchanged."""
    if name not in _CACHE:
        from deepinteract_amd import synth
        k, sizes, seeds = {**BATCHES, **TOPOLOGY_ONLY}[name]
        chains = [synth.synthetic_chain(n, s) for n, s in zip(sizes, seeds)]
        _CACHE[name] = (chains, _device_build(chains, k))
    return _CACHE[name]


def _ca(chain):
    return torch.as_tensor(np.ascontiguousarray(chain["backbone"][:, 1, :]), dtype=torch.float32)


# --------------------------------------------------------------------------- 1. kNN tie order
def _lattice(n, seed):
    """Small even integer coordinates (duplicates included): |x|^2, x.y and the expansion formula are
    exact in fp32 under any summation order or FMA use, so distances, ties and torch.topk's output
    are the same on every host."""
    rng = np.random.default_rng(seed)
    return torch.as_tensor(2.0 * rng.integers(0, 8, size=(n, 3)), dtype=torch.float32)


def _lattice_sets(case):
    if case == "all_tied":
        return [torch.full((70, 3), 6.0)]
    if case == "mixed":
        return [_lattice(200, 200), _lattice(300, 300)]
    return [_lattice(case[0], case[0])]


# (n, k): which branch of torch_topk_smallest the row takes
LATTICE_CASES = [
    ((200, 3), 3),     # partial_sort, k * 64 <= n
    ((192, 3), 3),     # partial_sort at the threshold itself, k * 64 == n
    ((1300, 20), 20),  # partial_sort, default k
    ((300, 20), 20),   # nth_element + std_sort over 19 elements (> 16: unguarded insertion tail)
    ((97, 30), 30),    # nth_element + std_sort over 29 elements
    ("all_tied", 20),  # partitioning on all-equal keys
    ("mixed", 20),     # two chains in one launch: the second chain's LDS slice and offsets
]


@pytest.mark.parametrize("case,k", LATTICE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_knn_tie_order_matches_torch_topk(case, k):
    """Exactly tied distances: indices and distances equal torch.topk's on the CPU (libstdc++
    partial_sort / nth_element + sort swap history, replayed by k_knn), bit for bit."""
    from deepinteract_amd.builder import knn
    from oracle import geot_oracle as O
    cas = _lattice_sets(case)
    idx, d2 = knn(cas, k)
    torch.cuda.synchronize()
    idx, d2 = idx.cpu().long(), d2.cpu()
    off = 0
    for ca in cas:
        n = ca.shape[0]
        d32 = O.pairwise_squared_distance(ca)
        d64 = O.pairwise_squared_distance(ca.double())
        assert torch.equal(d32.double(), d64)  # the inputs' premise: fp32 distances are exact
        ref_idx, ref_d2 = O.knn(ca, k)
        # the case reaches the replay and the replay matters: most rows (all of them at k >= 20)
        # have an exact tie in their top k + 1, and some rows are not in index order
        top = torch.topk(d32, min(k + 1, n), dim=1, largest=False).values
        tied = (top[:, 1:] == top[:, :-1]).any(1)
        by_index = torch.sort(d32, dim=1, stable=True).indices[:, :k]
        differ = int((by_index != ref_idx).any(1).sum())
        print(f"lattice {case} k={k} n={n}: {int(tied.sum())}/{n} rows tied, {differ} differ from index order")
        assert (bool(tied.all()) if k >= 20 else 2 * int(tied.sum()) > n) and differ > 0
        got_idx, got_d2 = idx[off:off + n], d2[off:off + n]
        bad = (got_idx != ref_idx).any(1)
        assert torch.equal(got_idx, ref_idx), f"{int(bad.sum())} of {n} rows differ, first row {int(bad.nonzero()[0])}"
        assert torch.equal(got_d2, ref_d2)
        off += n


# ------------------------------------------------------------- 2. kNN on random-walk chains
def _knn_chain_check(ca, idx, d2, k):
    """One chain's device kNN (idx [n,k], d2 [n,k], chain-local) against the float64 distance
    matrix. tol = 2 max|D32 - D64|: the reference's own deviation measured here, once for the
    device and once for the host. Returns the measured figures."""
    from oracle import geot_oracle as O
    n = ca.shape[0]
    d64 = O.pairwise_squared_distance(ca.double())
    d32 = O.pairwise_squared_distance(ca)
    tol = 2.0 * float((d32.double() - d64).abs().max())
    assert idx.shape == (n, k) and d2.shape == (n, k)
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] > srt[:, :-1]).all()), "a row repeats a neighbour"
    got64 = d64.gather(1, idx)
    want64 = torch.topk(d64, k, dim=1, largest=False).values  # ascending: sort(D64[i])[:k]
    e_rank = float((got64 - want64).abs().max())
    e_d2 = float((d2.double() - got64).abs().max())
    assert e_rank <= tol, (e_rank, tol)
    assert e_d2 <= tol, (e_d2, tol)
    # for the record: rows that differ from the host's oracle.knn, each explained by a near-tie at
    # its first differing rank r. Ranks < r agree, so the device's choice X sits at an oracle rank
    # > r with D32[X] - D32[oracle's choice] within the two deviations: top[r + 1] - top[r] <= tol
    ref_idx, _ = O.knn(ca, k)
    rows = (idx != ref_idx).any(1).nonzero().flatten().tolist()
    if rows:
        top = torch.topk(d32, min(k + 1, n), dim=1, largest=False).values.double()
        for i in rows:
            r = int((idx[i] != ref_idx[i]).nonzero()[0])
            assert r + 1 < top.shape[1], (i, r)
            gap = float(top[i, r + 1] - top[i, r])
            assert gap <= tol, f"row {i} differs from oracle.knn at rank {r} with a gap of {gap} > {tol}"
    return {"n": n, "tol": tol, "rank": e_rank, "d2": e_d2, "differ": len(rows)}


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_knn_against_float64(name):
    """Every row of every chain: indices valid and distinct, the r-th neighbour's float64 distance
    within tol of the r-th smallest, d2 within tol of the neighbour's float64 distance; rows that
    differ from the host's oracle.knn are counted and must be near-ties."""
    from deepinteract_amd.builder import knn
    chains, dev = _batch(name)
    k = dev["k"]
    idx2, d22 = knn([_ca(c) for c in chains], k)  # the stand-alone entry gives the batch's own kNN
    torch.cuda.synchronize()
    assert torch.equal(idx2.cpu().long(), dev["knn_idx"]) and torch.equal(d22.cpu(), dev["knn_d2"])
    differ = 0
    for g, chain in enumerate(chains):
        n0, n1 = dev["node_off"][g], dev["node_off"][g + 1]
        m = _knn_chain_check(_ca(chain), dev["knn_idx"][n0:n1], dev["knn_d2"][n0:n1], k)
        differ += m["differ"]
        print(f"kNN {name} chain {g} n={m['n']} k={k}: tol {m['tol']:.3e}, rank err {m['rank']:.3e}, "
              f"d2 err {m['d2']:.3e}, rows differing from oracle.knn {m['differ']}")
    print(f"kNN {name}: {differ} rows differ from oracle.knn")


def test_knn_rejects_chain_shorter_than_k():
    from deepinteract_amd.builder import knn
    with pytest.raises(ValueError):
        knn([_lattice(40, 1), _lattice(19, 2)], 20)


# ------------------------------------------------------------------------------- 3. topology
@pytest.mark.parametrize("name", sorted(BATCHES) + sorted(TOPOLOGY_ONLY))
def test_topology_exact(name):
    """[DGL-ASSUMPTION] edge e = v k + r: dst = v, src = knn_idx[v, r] + the chain's node offset;
    in_ptr[v] = v k up to and including v = Nt; node_pos = the node's index inside its chain."""
    _, dev = _batch(name)
    k, sizes = dev["k"], dev["sizes"]
    nt = sum(sizes)
    chain_off = torch.repeat_interleave(torch.as_tensor(dev["node_off"][:-1]), torch.as_tensor(sizes))
    assert dev["dst"].shape == (nt * k,) and dev["src"].shape == (nt * k,)
    assert torch.equal(dev["dst"], torch.arange(nt * k) // k)
    assert torch.equal(dev["src"], (dev["knn_idx"] + chain_off[:, None]).reshape(-1))
    assert dev["in_ptr"].shape == (nt + 1,) and torch.equal(dev["in_ptr"], torch.arange(nt + 1) * k)
    assert torch.equal(dev["node_pos"], torch.arange(nt) - chain_off)


# ------------------------------------------------------------------------------- 4. features
def _features(chain, idx, d2, dtype):
    """Node columns 0-6 and edge columns 0-19, 27 as oracle.build_graph writes them, evaluated in
    `dtype` from the given kNN (idx [N,k] int64 chain-local, d2 [N,k])."""
    from oracle import geot_oracle as O
    bb = torch.as_tensor(np.asarray(chain["backbone"])).to(dtype)
    n, k = idx.shape
    ca = bb[:, 1, :]
    src = idx.reshape(-1)
    dst = torch.arange(n).repeat_interleave(k)
    node_geo = O.dihedrals(bb.reshape(1, n, 4, 3))[0]
    pos = O.minmax(torch.arange(n, dtype=dtype)).reshape(-1, 1)
    rbf = O.rbf(d2.to(dtype).reshape(1, n, k))[0].reshape(-1, O.NUM_RBF)
    pos_e = torch.sin((src - dst).to(dtype)).reshape(-1, 1)
    w = O.minmax(torch.sum((ca[src] - ca[dst]) ** 2, 1)).reshape(-1, 1)
    am = torch.as_tensor(np.asarray(chain["amide_norm"])).to(dtype)
    v1, v2 = am[dst], am[src]
    cosang = (v1 * v2).sum(-1) / (torch.linalg.norm(v1, dim=-1) * torch.linalg.norm(v2, dim=-1))
    ang = torch.nan_to_num(torch.acos(cosang), nan=0.0)
    ang = torch.nan_to_num(O.minmax(ang), nan=0.0).reshape(-1, 1)
    return torch.cat((pos, node_geo), 1).double(), torch.cat((pos_e, w, rbf), 1).double(), ang.double()


def _feature_chain_check(chain, dev, g):
    """Chain g of a device build against the float64 evaluation fed with the device's own kNN."""
    n0, n1 = dev["node_off"][g], dev["node_off"][g + 1]
    e0, e1 = dev["edge_off"][g], dev["edge_off"][g + 1]
    idx, d2 = dev["knn_idx"][n0:n1], dev["knn_d2"][n0:n1]
    nf, ef = dev["node_f"][n0:n1], dev["edge_f"][e0:e1]
    node64, edge64, ang64 = _features(chain, idx, d2, torch.float64)
    # the condition on the inputs: the fp32 oracle formulas sit within half of each bound
    node32, edge32, ang32 = _features(chain, idx, d2, torch.float32)
    o_node = float((node32 - node64).abs().max())
    o_edge = float((edge32 - edge64).abs().max())
    o_ang = float((ang32 - ang64).abs().max())
    assert o_node <= NODE_TOL / 2 and o_edge <= EDGE_TOL / 2 and o_ang <= AMIDE_TOL / 2, (o_node, o_edge, o_ang)
    assert bool(torch.isfinite(nf).all()) and bool(torch.isfinite(ef).all())
    e_node = float((nf[:, :7].double() - node64).abs().max())
    e_edge = float((ef[:, :20].double() - edge64).abs().max())
    e_ang = float((ef[:, 27:28].double() - ang64).abs().max())
    assert torch.equal(ef[:, 20:27], torch.tensor(GEO_REF).expand(e1 - e0, 7))
    assert torch.equal(nf[:, 7:], torch.as_tensor(np.asarray(chain["dips"]), dtype=torch.float32))
    return {"node": e_node, "edge": e_edge, "amide": e_ang, "o_node": o_node, "o_edge": o_edge, "o_amide": o_ang}


def _assert_feature_bounds(m, what):
    assert m["node"] <= NODE_TOL, (what, m)
    assert m["edge"] <= EDGE_TOL, (what, m)
    assert m["amide"] <= AMIDE_TOL, (what, m)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_features_against_float64(name):
    """Per-chain min/max statistics, RBF, dihedral padding (phi[0], psi[-1], omega[-1] = 0), sin,
    edge weight and amide columns of every chain, independently of the kNN."""
    chains, dev = _batch(name)
    worst = {}
    for g, chain in enumerate(chains):
        m = _feature_chain_check(chain, dev, g)
        print(f"features {name} chain {g} n={dev['sizes'][g]}: device node {m['node']:.3e} edge0-19 {m['edge']:.3e} "
              f"amide {m['amide']:.3e} | fp32 oracle node {m['o_node']:.3e} edge {m['o_edge']:.3e} "
              f"amide {m['o_amide']:.3e}")
        _assert_feature_bounds(m, (name, g))
        worst = {key: max(val, worst.get(key, 0.0)) for key, val in m.items()}
    print(f"features {name} worst: " + ", ".join(f"{key} {val:.3e}" for key, val in worst.items()))


def test_degenerate_amide_chains_do_not_leak():
    """A chain whose amide normals are all zero (angle NaN -> 0, range 0: column exactly 0) and one
    with about 10 % zero normals (synth's GLY rule plus every 20th residue), between ordinary chains:
    every chain's features equal, bit for bit, those of the same chain built alone, so no chain's
    min/max statistics reach another's columns."""
    from deepinteract_amd import synth
    k = 20
    chains = [synth.synthetic_chain(n, 7000 + g) for g, n in enumerate([64, 50, 300, 97])]
    chains[1]["amide_norm"][:] = 0.0
    chains[2]["amide_norm"][::20] = 0.0
    frac = float((np.abs(chains[2]["amide_norm"]).sum(1) == 0).mean())
    assert 0.05 <= frac <= 0.15, frac
    dev = _device_build(chains, k)
    e0, e1 = dev["edge_off"][1], dev["edge_off"][2]
    assert bool((dev["edge_f"][e0:e1, 27] == 0).all())
    for g, chain in enumerate(chains):
        m = _feature_chain_check(chain, dev, g)
        print(f"degenerate amide batch chain {g}: node {m['node']:.3e} edge0-19 {m['edge']:.3e} amide {m['amide']:.3e}")
        _assert_feature_bounds(m, g)
        alone = _device_build([chain], k)
        n0, n1 = dev["node_off"][g], dev["node_off"][g + 1]
        a0, a1 = dev["edge_off"][g], dev["edge_off"][g + 1]
        assert torch.equal(dev["knn_idx"][n0:n1], alone["knn_idx"]) and torch.equal(dev["knn_d2"][n0:n1], alone["knn_d2"])
        assert torch.equal(dev["node_f"][n0:n1], alone["node_f"]), g
        assert torch.equal(dev["edge_f"][a0:a1], alone["edge_f"]), g


# -------------------------------------------------------------------------- 5. neighbour ids
def _nbr_check(sizes, k, seeds, oracle_seeds=None, base_seed=9000):
    """Device torch-seeded neighbour ids of a batch against oracle.build_graph's src_nbr / dst_nbr
    (torch.randperm on the host after manual_seed) plus the chain's edge offset."""
    from deepinteract_amd import synth
    from oracle import geot_oracle as O
    chains = [synth.synthetic_chain(n, base_seed + g) for g, n in enumerate(sizes)]
    dev = _device_build(chains, k, nbr_seeds=seeds)
    for g, chain in enumerate(chains):
        ref = O.build_graph(chain, k=k, seed=(oracle_seeds or seeds)[g])
        e0, e1 = dev["edge_off"][g], dev["edge_off"][g + 1]
        n0 = dev["node_off"][g]
        nbr = dev["nbr"][e0:e1]
        # the kept randperm positions alone (independent of the kNN), then the ids themselves
        pos = torch.cat([nbr[:, :2] - dev["src"][e0:e1, None] * k, nbr[:, 2:] - dev["dst"][e0:e1, None] * k], 1)
        ref_pos = torch.cat([ref["src_nbr"] - ref["src"][:, None] * k, ref["dst_nbr"] - ref["dst"][:, None] * k], 1)
        assert torch.equal(pos, ref_pos), (g, sizes[g], int((pos != ref_pos).any(1).sum()))
        assert torch.equal(dev["src"][e0:e1] - n0, ref["src"]), g
        assert torch.equal(nbr, torch.cat([ref["src_nbr"], ref["dst_nbr"]], 1) + e0), g


def test_nbr_ids_k30():
    _nbr_check([30, 97, 400], 30, [21, 22, 23])


def test_nbr_ids_k4_calls_aligned_to_mt_blocks():
    """k - 1 = 3 divides 624: no randperm call straddles an mt19937 block."""
    _nbr_check([40, 9], 4, [31, 32])


def test_nbr_ids_eight_chains_one_wave_each():
    _nbr_check([20, 1000, 21, 333, 64, 777, 150, 500], 20, [41, 42, 43, 44, 45, 46, 47, 48])


def test_nbr_ids_seed_uses_low_32_bits():
    """torch seeds mt19937 from the low 32 bits of the seed: 2**32 + 5 draws what 5 draws."""
    g = torch.Generator()
    a = torch.randperm(20, generator=g.manual_seed(2 ** 32 + 5))
    b = torch.randperm(20, generator=g.manual_seed(5))
    assert torch.equal(a, b)  # the premise, on this host's torch
    _nbr_check([64, 33], 20, [2 ** 32 + 5, 5], oracle_seeds=[5, 5])
