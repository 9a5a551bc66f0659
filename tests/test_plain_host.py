"""disable_geometric_mode (the reference's plain Graph Transformer baseline) on the host: key set,
the float64 restatement against the reference's own outputs, packing, blob sizes, the C entry points'
refusals, configuration inference and checkpoint loading. No GPU.

The fixture tests/golden/plain_tiny.npz comes from the reference's unmodified
LitGINI(disable_geometric_mode=True) (tests/golden/make_golden_plain.py).

The attention clamps: tests/golden/sat_tiny.npz's plain half is the reference under plain_cases'
saturating weights, which plain_forward64 must match as it matches plain_tiny.npz while each wrong
clamp placement misses it by 100 times the bound; and the conditions on the saturating inputs of
tests/test_gpu_geot_saturated.py's plain tests, as tests/test_geot_cases_host.py states them."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import geot_cases as C
import plain_cases as P
from blob_emulator import _unpack
from deepinteract_amd import _lib, packing
from deepinteract_amd.config import GeoTConfig
from deepinteract_amd.weights import (check_state_dict, geot_keys, infer_config, read_checkpoint,
                                      reference_init_state_dict, seeded_state_dict, state_dict_sha256)

DI_DT = {"f32": _lib.DI_F32, "bf16": _lib.DI_BF16}


def _rel(got, ref):
    """normwise error: max |got - ref| / max |ref|"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def test_geot_keys_equal_the_references():
    z = P.fixture()
    cfg = P.plain_cfg(2)
    keys = geot_keys(cfg)
    assert [k for k, _, _ in keys] == list(z["geot_key_names"]) and len(keys) == 58
    assert [",".join(str(d) for d in s) for _, s, _ in keys] == list(z["geot_key_shapes"])
    names = {k for k, _, _ in keys}
    assert "gnn_module.0.init_edge_module.weight" in names
    assert not any("node_embedding" in k or "gt_block.0.conformation_module" in k for k in names)
    assert [k for k in names if "conformation_module" in k] == ["gnn_module.0.gt_block.1.conformation_module.weight"]
    assert not any(k.endswith(("Q.bias", "K.bias", "V.bias", "edge_feats_projection.bias")) for k in names)
    assert str(z["weights_sha256"]) == state_dict_sha256(seeded_state_dict(0, cfg))
    # the default key set is what it was
    assert len(geot_keys(GeoTConfig())) == len(geot_keys(GeoTConfig(disable_geometric_mode=False))) > 58


def test_reference_init_follows_the_key_set():
    sd = reference_init_state_dict(0, P.plain_cfg(2), with_head=False)
    assert check_state_dict(sd, P.plain_cfg(2), with_head=False) == []
    for k in ("gnn_module.0.init_edge_module.weight", "gnn_module.0.gt_block.1.conformation_module.weight"):
        w = sd[k]
        assert tuple(w.shape) == (128, 30)
        # glorot_orthogonal(scale=2): var(W) = 2 / (fan_in + fan_out)
        assert abs(float(w.var()) * (128 + 30) / 2.0 - 1.0) < 1e-4


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_plain_forward64_matches_the_reference(tag):
    """Every stored stage within 1e-5 (normwise) of the reference's fp32 outputs."""
    z = P.fixture()
    sd = seeded_state_dict(0, P.plain_cfg(2), with_head=False)
    item = P.fixture_item(z, tag)
    assert item["src"].numel() in (660, 420) and item["src"].numel() % 64 != 0
    node, edge, inter = P.plain_forward64(sd, item, 2, key=("fixture", tag), return_intermediates=True)
    stages = [("node_out", node, None), ("layer0_node", inter["node0"], None),
              ("init_edge", inter["init_edge"], z[f"{tag}_init_edge_rows"]),
              ("layer0_edge", inter["edge0"], z[f"{tag}_layer0_edge_rows"]),
              ("edge_out", edge, z[f"{tag}_edge_rows"])]
    for name, got, rows in stages:
        ref = z[f"{tag}_{name}"].astype(np.float64)
        if rows is not None:
            assert rows[-1] == got.shape[0] - 1  # the chain's last row is among the samples
            colsum = z[f"{tag}_{name}_colsum"]
            assert np.abs(got.sum(0) - colsum).max() <= 1e-5 * np.abs(got).sum(0).max(), name
            got = got[rows]
        err = _rel(got, ref)
        print(f"plain_forward64 vs reference {tag} {name}: {err:.3e}")
        assert err < 1e-5, (name, err)
    assert np.array_equal(inter["edge0"], edge)  # the returned edges are the last intermediate layer's


def test_l1_returns_f0():
    """L = 1: the only layer is the final one, so the returned edge features are InitEdge's F0 = W_i .
    cat(G[:, 0], G[:, 1], G), here evaluated column by column."""
    from oracle import geot_oracle as O
    sd = P.state_dict(1)
    item = P.fixture_item(P.fixture(), "g2")
    node, edge = P.plain_forward64(sd, item, 1)
    G = item["edge_f"].double()
    f0 = (G[:, :1] * sd["gnn_module.0.init_edge_module.weight"][:, 0].double()
          + G[:, 1:2] * sd["gnn_module.0.init_edge_module.weight"][:, 1].double()
          + O._lin(G, {"w.weight": sd["gnn_module.0.init_edge_module.weight"][:, 2:].double()}, "w"))
    assert _rel(edge, f0.numpy()) < 1e-12
    assert node.shape == (21, 128) and np.isfinite(node).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_blobs_hold_the_folded_matrices_rounded_once(dtype):
    sd = P.state_dict(2)
    rnd = (lambda x: packing._bf16_round(x)) if dtype == "bf16" else \
        (lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64))
    npd = packing._np
    # InitEdge: the doubled columns folded in fp64
    wi = npd(sd["gnn_module.0.init_edge_module.weight"])
    want = np.zeros((128, 32))
    want[:, :28] = wi[:, 2:]
    want[:, 0] += wi[:, 0]
    want[:, 1] += wi[:, 1]
    mat, vec = packing.init_blob_plain(sd, dtype)
    assert vec.numel() == 0 and mat.numel() == packing.PI_NBLK * 512
    assert np.array_equal(_unpack(mat, 0, 128, 32, dtype), rnd(want))
    # intermediate layer
    p = "gnn_module.0.gt_block.0"
    mat, vec = packing.edge_blob_plain(sd, 0, False, dtype)
    assert (mat.numel() // 512, vec.numel()) == packing.PLAIN_BLOB_SIZES[1] == (192, 512)
    s, t = packing.bn_affine(sd, f"{p}.batch_norm1_edge_feats")
    wp, bp = packing.fold_bn_before(*packing.lin(sd, f"{p}.mha_module.edge_feats_projection"), s, t)
    assert np.abs(bp).max() > 0  # the bias-free projection gets a bias from the fold
    assert np.array_equal(_unpack(mat, packing.PL_P, 128, 128, dtype), rnd(wp))
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)  # noqa: E731
    v = vec.numpy()
    assert np.array_equal(v[0:128], f32(bp))
    wo, bo = packing.lin(sd, f"{p}.O_edge_feats")
    assert np.array_equal(_unpack(mat, packing.PL_OE, 128, 128, dtype), rnd(wo)) and np.array_equal(v[128:256], f32(bo))
    s, t = packing.bn_affine(sd, f"{p}.batch_norm2_edge_feats")
    w1, b1 = packing.fold_bn_before(*packing.lin(sd, f"{p}.edge_feats_MLP.0"), s, t)
    for half in range(2):
        assert np.array_equal(_unpack(mat, packing.PL_F1 + 32 * half, 128, 128, dtype), rnd(w1[128 * half:128 * half + 128]))
        w2 = npd(sd[f"{p}.edge_feats_MLP.3.weight"])[:, 128 * half:128 * half + 128]
        assert np.array_equal(_unpack(mat, packing.PL_F2 + 32 * half, 128, 128, dtype), rnd(w2))
    assert np.array_equal(v[256:512], f32(b1))
    # final layer: W_c's columns as [G, F[:,0], F[:,1], 0, 0]
    p = "gnn_module.0.gt_block.1"
    mat, vec = packing.edge_blob_plain(sd, 1, True, dtype)
    assert (mat.numel() // 512, vec.numel()) == packing.PLAIN_BLOB_SIZES[2] == (40, 128)
    wc = npd(sd[f"{p}.conformation_module.weight"])
    want = np.zeros((128, 32))
    want[:, :28], want[:, 28:30] = wc[:, 2:], wc[:, :2]
    assert np.array_equal(_unpack(mat, packing.PF_WC, 128, 32, dtype), rnd(want))
    s, t = packing.bn_affine(sd, f"{p}.batch_norm1_edge_feats")
    wp, bp = packing.fold_bn_before(*packing.lin(sd, f"{p}.mha_module.edge_feats_projection"), s, t)
    assert np.array_equal(_unpack(mat, packing.PF_P, 128, 128, dtype), rnd(wp)) and np.array_equal(vec.numpy(), f32(bp))


def test_packed_geot_builds_plain_blobs_and_keeps_the_rest():
    sd = P.state_dict(2)
    pk = packing.PackedGeoT(sd, "bf16", P.plain_cfg(2))
    assert pk.plain and pk.pos_src is None and pk.num_layers == 2
    assert [m.numel() // 512 for m, _ in pk.edge] == [192, 40] and pk.init[0].numel() == 8 * 512
    assert pk.embed[0].numel() == packing.EM_NBLK * 512 and [m.numel() // 512 for m, _ in pk.node] == [256, 160]
    assert len(packing.BLOB_SIZES) == 7
    assert not packing.PackedGeoT(seeded_state_dict(0, with_head=False), "f32").plain


def test_blob_sizes_equal_the_librarys():
    lib = _lib.load()
    assert lib.di_abi_version() == 8
    for kind, (nblk, nvec) in packing.PLAIN_BLOB_SIZES.items():
        for dtype, esz in (("f32", 4), ("bf16", 2)):
            assert lib.di_plain_blob_bytes(kind, DI_DT[dtype], 0) == nblk * 512 * esz
            assert lib.di_plain_blob_bytes(kind, DI_DT[dtype], 1) == nvec * 4
    for kind in (-1, 3, 7):
        assert lib.di_plain_blob_bytes(kind, _lib.DI_F32, 0) == -1
    assert lib.di_plain_blob_bytes(1, 5, 0) == -1
    assert lib.di_blob_bytes(7, _lib.DI_F32, 0) == -1 and lib.di_blob_layout(7, _lib.DI_BF16) == -1


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(16)  # never dereferenced on these paths
    G = _lib.DiGraph
    good = G(8, 16, 16, 16, 16, 16, 16, 0)
    gp = ctypes.byref(good)
    init_args = [gp, 1, p, p, p, None]
    for i in (0, 2, 3, 4):  # graph, edge_f, wmat, f_out
        a = list(init_args)
        a[i] = None
        assert lib.di_init_edge_plain(*a) == -1, i
    assert lib.di_init_edge_plain(gp, 7, p, p, p, None) == -1
    assert lib.di_init_edge_plain(gp, -1, p, p, p, None) == -1
    layer_args = [gp, 0, 0, p, p, p, p, p, p, p, None]
    for final in (0, 1):
        for i in (0, 3, 4, 5, 6, 7, 8):  # graph, edge_f, f_in, qkv, wmat, wvec, alpha_out
            a = list(layer_args)
            a[2], a[i] = final, None
            assert lib.di_edge_layer_plain(*a) == -1, (final, i)
        assert lib.di_edge_layer_plain(gp, 2, final, p, p, p, p, p, p, p, None) == -1
    assert lib.di_edge_layer_plain(gp, 1, 0, p, p, p, p, p, p, None, None) == -1  # f_out on a non-final layer
    for bad in (G(8, 0, 16, 16, 16, 16, 16, 0), G(8, -3, 16, 16, 16, 16, 16, 0)):
        assert lib.di_init_edge_plain(ctypes.byref(bad), 1, p, p, p, None) == -1
        assert lib.di_edge_layer_plain(ctypes.byref(bad), 1, 1, p, p, p, p, p, p, None, None) == -1
    for bad in (G(8, 16, None, 16, 16, 16, 16, 0), G(8, 16, 16, None, 16, 16, 16, 0)):  # src / dst
        assert lib.di_edge_layer_plain(ctypes.byref(bad), 1, 1, p, p, p, p, p, p, None, None) == -1


def _write_ckpt(path, sd, **extra_hp):
    hp = {"num_node_input_feats": 113, "gnn_activ_fn": torch.nn.SiLU(), "num_gnn_layers": 2,
          "num_gnn_hidden_channels": 128, "num_gnn_attention_heads": 4, "knn": 20, "num_interact_layers": 14,
          "num_interact_hidden_channels": 128, "lr": 1e-3}
    hp.update(extra_hp)
    torch.save({"state_dict": sd, "hyper_parameters": hp}, path)


def test_infer_config_and_checkpoints(tmp_path):
    from deepinteract_amd.modules import DGLGeometricTransformer, LitGINI
    plain_sd = seeded_state_dict(0, P.plain_cfg(2))
    geo_sd = seeded_state_dict(0)
    cfg = infer_config(plain_sd)
    assert cfg.disable_geometric_mode and cfg.num_gnn_layers == 2 and cfg.node_count_limit == 2304
    assert infer_config(plain_sd, max_num_graph_nodes=4096).node_count_limit == 4096
    assert check_state_dict(plain_sd, cfg) == []
    assert not infer_config(geo_sd).disable_geometric_mode
    assert infer_config(geo_sd, disable_geometric_mode=True).disable_geometric_mode
    assert not infer_config(plain_sd, disable_geometric_mode=False).disable_geometric_mode
    # a saved checkpoint whose hyper-parameters carry the flag
    path = os.path.join(tmp_path, "plain.ckpt")
    _write_ckpt(path, plain_sd, disable_geometric_mode=True)
    _, arch = read_checkpoint(path)
    assert arch["disable_geometric_mode"] is True
    m = LitGINI.load_from_checkpoint(path)
    assert m.cfg.disable_geometric_mode and "gnn_module.0.init_edge_module.weight" in m._geot_sd
    # without the hyper-parameter the key decides
    _write_ckpt(path, plain_sd)
    assert LitGINI.load_from_checkpoint(path).cfg.disable_geometric_mode
    # a plain state dict into a geometric model, and the reverse: the strict check's message
    with pytest.raises(RuntimeError, match="state dict does not match LitGINI"):
        LitGINI.load_from_checkpoint(path, disable_geometric_mode=False)
    _write_ckpt(path, geo_sd)
    assert not LitGINI.load_from_checkpoint(path).cfg.disable_geometric_mode
    with pytest.raises(RuntimeError, match="state dict does not match LitGINI"):
        LitGINI.load_from_checkpoint(path, disable_geometric_mode=True)
    _write_ckpt(path, geo_sd, disable_geometric_mode=True)
    with pytest.raises(RuntimeError, match="state dict does not match LitGINI"):
        LitGINI.load_from_checkpoint(path)
    assert LitGINI(disable_geometric_mode=True).cfg.disable_geometric_mode and not LitGINI().cfg.disable_geometric_mode
    assert DGLGeometricTransformer(disable_geometric_mode=True).cfg.disable_geometric_mode


def test_fold_attn_and_overlapped_schedule_are_refused():
    from deepinteract_amd.engine import GeoTEngine
    from deepinteract_amd.pipeline import OverlappedSchedule
    eng = GeoTEngine.__new__(GeoTEngine)  # the refusal comes before anything touches a device
    eng.plain, eng.fold_attn = True, True
    with pytest.raises(ValueError, match="fold_attn"):
        eng.forward(None)
    fake = types.SimpleNamespace(plain=True, dtype="bf16", fuse_embed_init=True, resident_init=False)
    with pytest.raises(NotImplementedError, match="disable_geometric_mode"):
        OverlappedSchedule(fake, [], [], [], [], [], [])


@pytest.mark.parametrize("tag", ["g1", "g2"])
def test_saturated_fixture_pins_the_clamp_order(tag):
    z = np.load(C.SAT_GOLDEN)
    sd = C.scale_attention(seeded_state_dict(P.SAT_SEED, P.plain_cfg(2)), P.block_factors(2))
    assert str(z["plain_weights_sha256"]) == state_dict_sha256(sd)
    assert z["plain_factors"].tolist() == [[li, *P.block_factors(2)[li]] for li in range(2)]
    it = C.fixture_item(z, tag)
    node, edge, tails, inter = P.variant64(sd, it, 2, return_intermediates=True)
    n64, e64 = P.plain_forward64(sd, it, 2)
    assert np.array_equal(node, n64) and np.array_equal(edge, e64)  # the reference setting IS oracle.mha
    errs = C.sat_stage_errors(z, "plain", tag, node, edge, inter)
    print(f"plain_forward64 vs saturated reference {tag}: {errs}")
    assert max(errs.values()) < 1e-5, errs
    for t in tails:
        print(f"{tag} {t['layer']}: tail fractions {C.tail_fractions(t)}")
        assert all(t[k] > 0 for k in C.TAILS), t
    for m, switches in C.MUTANTS.items():
        mn, me, _, minter = P.variant64(sd, it, 2, return_intermediates=True, **switches)
        merr = C.sat_stage_errors_unchecked(z, "plain", tag, mn, me, minter)
        print(f"{tag} mutant {m}: {merr}")
        assert max(merr["node_out"], merr["layer0_node"], merr["layer0_edge"], merr["edge_out"]) >= 100 * 1e-5, (m, merr)


# the chains tests/test_gpu_geot_saturated.py's plain tests run (tests/test_gpu_plain.py's batches)
SAT_CASES = {k: v for k, v in C.host_cases().items() if k != "ragged_general"}
SAT_CHAINS = [(name, g) for name, items in SAT_CASES.items() for g in range(len(items))]


def test_saturating_factors_apply_per_role():
    for L in C.LAYERS:
        f = P.block_factors(L)
        assert sorted(f) == list(range(L)) and f[L - 1] == P.SAT_FACTORS[L - 1][1]
        assert all(f[li] == P.SAT_FACTORS[li][0] for li in range(L - 1))
        base, sat = P.state_dict(L, P.SAT_SEED), P.saturating_state_dict(L)
        changed = {k for k in base if not torch.equal(base[k], sat[k])}
        assert changed == {f"gnn_module.0.gt_block.{li}.mha_module.{m}.weight" for li in range(L)
                           for m, s in (("Q", f[li][0]), ("K", f[li][0]), ("edge_feats_projection", f[li][1])) if s != 1.0}


@pytest.mark.parametrize("L", C.LAYERS)
@pytest.mark.parametrize("name,g", SAT_CHAINS)
def test_saturating_case_conditions(name, g, L):
    """Tails, conditioning, rows and decisive mutants of one (chain, L), geot_cases' checkers."""
    sd, item = P.saturating_state_dict(L), SAT_CASES[name][g]
    node, edge, tails = P.variant64(sd, item, L)
    n64, e64 = P.plain_forward64(sd, item, L, key=("host-sat", name, g))
    assert np.array_equal(node, n64) and np.array_equal(edge, e64)
    for t in tails:
        print(f"plain {name} chain {g} L={L} {t['layer']}: " + ", ".join(f"{k} {f:.3f}" for k, f in zip(C.TAILS, C.tail_fractions(t))))
    C.check_tail_window(name, tails)
    with torch.no_grad():
        n32, e32 = P.plain_forward(sd, item, L)
    en, ee = C.check(n32.numpy(), n64)[0], C.check(e32.numpy(), e64)[0]
    assert max(en, ee) <= 1e-5, (en, ee)
    for what, ref in (("node", n64), ("edge", e64)):
        ratio = np.abs(ref).max(axis=1) / np.abs(ref).max()
        assert ratio.min() >= 0.1, (what, int(ratio.argmin()), float(ratio.min()))
    sat = P.bf16_sensitivity(sd, item, L)
    seeded = P.bf16_sensitivity(P.state_dict(L, P.SAT_SEED), item, L)
    bounds = C.sat_bounds("bf16", sat, seeded)
    errors = C.mutant_errors(P.plain_forward, sd, item, L, (n64, e64))
    print(f"plain {name} chain {g} L={L}: fp32 vs fp64 {max(en, ee):.2e}; bf16 sensitivity saturating {sat[0]:.2e} / {sat[1]:.2e}, "
          f"seeded {seeded[0]:.2e} / {seeded[1]:.2e}, bf16 bounds {bounds[0]:.2e} / {bounds[1]:.2e}; mutants "
          + ", ".join(f"{m} {a:.2e} / {b:.2e}" for m, (a, b) in errors.items()))
    C.check_decisive(name, errors, bounds)
