"""InitEdge's edge output kept as its 32-wide factor z0 (di_embed_init_edge_z) and layer 0's edge
kernel rebuilding F0 = combined_linear_2(z0) in registers (di_edge_layer_z), against the F path
(di_embed_init_edge + di_edge_layer), bf16 reference-featurised batches:

* kernel level, bit identity: layer 0's F rows and alpha, and the embedding's h / Q,K,V, torch.equal on
  the smallest batches that reach each way the tile code can go wrong -- a single partial 256-edge
  tile whose last waves are all clamped rows (Et = 420), a last valid row inside a wave (Et = 324),
  whole tiles only (Et = 1280), and more tiles than CUs (some blocks run two tiles: the resident
  combined_linear_2 blocks, the z0 reload and the ring's carry-over across tiles);
* the factor itself: z0 decoded on the host (the row layout of csrc/mfma32.h) times the state dict's
  combined_linear_2 weight in fp32, rounded to bf16, within 1 bf16 ulp of the F path's F0 (the MFMA
  adds in another order than torch, so this one is not exact; it catches a wrong row / half layout);
* engine level: GeoTEngine.forward with z_init on and off, 2 and 4 layers, every output torch.equal;
  one layer, fp32, a batch without DI_GRAPH_GEO_REF and the folded aggregation keep the F path;
* the entry points refuse fp32, graphs without DI_GRAPH_GEO_REF and null z / init_wmat on the host
  (no launch: that test needs no GPU).
"""
import ctypes

import pytest
import torch

K = 20
Z_ROW = 32


def _batch(sizes, k=K, seed0=7000):
    from deepinteract_amd import synth
    from deepinteract_amd.builder import build_graph_batch
    chains = [synth.synthetic_chain(n, seed0 + i) for i, n in enumerate(sizes)]
    return build_graph_batch(chains, k=k, nbr_seeds=list(range(1, len(sizes) + 1)))


@pytest.fixture(scope="module")
def sd():
    from deepinteract_amd.weights import seeded_state_dict
    return seeded_state_dict(0, with_head=False)


@pytest.fixture(scope="module")
def eng(sd):
    from deepinteract_amd.engine import GeoTEngine
    return GeoTEngine(sd, "bf16")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _layer0(eng, gb, use_z):
    """The embedding + InitEdge launch and layer 0's edge layer through the C ABI ->
    dict(h, qkv, edge (F0 or z0), alpha, f1); every output pre-filled with NaN."""
    from deepinteract_amd import _lib
    lib, p, dev = eng.lib, eng.packed, gb.node_f.device
    nt, et = gb.num_nodes, gb.num_edges
    bf = dict(dtype=torch.bfloat16, device=dev)
    nan = float("nan")
    o = {"h": torch.full((nt, 128), nan, **bf), "qkv": torch.full((nt, 384), nan, **bf),
         "edge": torch.full((et, Z_ROW if use_z else 128), nan, **bf),
         "alpha": torch.full((et, 4), nan, device=dev), "f1": torch.full((et, 128), nan, **bf)}
    g = ctypes.byref(gb.c_graph)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    em, ev = p.edge[0]
    init = lib.di_embed_init_edge_z if use_z else lib.di_embed_init_edge
    assert init(g, _lib.DI_BF16, gb.node_f.shape[1], _p(gb.node_f), _p(p.embed[0]), _p(p.embed[1]), _p(o["h"]),
                _p(o["qkv"]), _p(gb.edge_f), _p(p.init[0]), _p(p.init[1]), _p(p.pos_src), _p(p.pos_dst), _p(o["edge"]),
                None, -1, st) == 0
    if use_z:
        rc = lib.di_edge_layer_z(g, _lib.DI_BF16, _p(gb.edge_f), _p(o["edge"]), _p(p.init[0]), _p(o["qkv"]), _p(em),
                                 _p(ev), _p(o["alpha"]), _p(o["f1"]), st)
    else:
        rc = lib.di_edge_layer(g, _lib.DI_BF16, 0, _p(gb.edge_f), _p(o["edge"]), None, _p(o["qkv"]), _p(em), _p(ev),
                               _p(o["alpha"]), _p(o["f1"]), None, st)
    assert rc == 0
    torch.cuda.synchronize()
    return o


def _more_tiles_than_cus():
    """Chain sizes whose edges fill more 256-edge tiles than the device has CUs (two chains of 1,650
    residues on 256 CUs: 258 tiles)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if -(-2 * 1650 * K // 256) > cus:
        return [1650, 1650], cus
    need = ((cus + 2) * 256 + K - 1) // K  # residues for cus + 2 tiles
    n = max(2, -(-need // 2000))
    return [-(-need // n)] * n, cus


# (chain sizes, k, expected Et)
SHAPES = {"partial_tile_clamped_waves": ([21], 20, 420), "last_row_inside_a_wave": ([13, 14], 12, 324),
          "whole_tiles": ([64], 20, 1280)}

_f_path = {}


def _pair(eng, name):
    """(batch, F-path outputs, z-path outputs) of a named shape, computed once."""
    if name not in _f_path:
        if name == "two_tiles_per_block":
            sizes, cus = _more_tiles_than_cus()
            gb = _batch(sizes)
            assert -(-gb.num_edges // 256) > cus
        else:
            sizes, k, et = SHAPES[name]
            gb = _batch(sizes, k)
            assert gb.num_edges == et
        assert gb.geo_ref
        _f_path[name] = (gb, _layer0(eng, gb, False), _layer0(eng, gb, True))
    return _f_path[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES) + ["two_tiles_per_block"])
def test_layer0_bit_identical(eng, name):
    gb, ref, got = _pair(eng, name)
    for key in ("h", "qkv", "alpha", "f1"):
        assert torch.isfinite(ref[key].float()).all(), key
        assert torch.equal(ref[key], got[key]), (name, key, int((ref[key] != got[key]).sum()))
    assert torch.isfinite(got["edge"].float()).all()  # every z0 row written


def z0_feature_order():
    """Element index of a z0 row -> z0 feature (csrc/mfma32.h): element 16 h + 8 s + j is feature
    16 s + 8 (j >> 2) + 4 h + (j & 3)."""
    feat = torch.empty(Z_ROW, dtype=torch.long)
    for h in range(2):
        for s in range(2):
            for j in range(8):
                feat[16 * h + 8 * s + j] = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)
    assert sorted(feat.tolist()) == list(range(Z_ROW))
    return feat


@pytest.mark.gpu
def test_z0_is_the_factor_of_f0(eng, sd):
    gb, ref, got = _pair(eng, "partial_tile_clamped_waves")
    z = torch.empty_like(got["edge"])
    z[:, z0_feature_order().to(z.device)] = got["edge"]  # natural feature order
    w = torch.zeros(128, Z_ROW)
    w28 = sd["gnn_module.0.init_edge_module.combined_linear_2.weight"]
    w[:, :w28.shape[1]] = w28
    w = w.bfloat16().to(z.device)
    assert (z[:, w28.shape[1]:] == 0).all()  # the padding features
    f0 = (z.float() @ w.float().t()).bfloat16().float()
    want = ref["edge"].float()
    # 1 bf16 ulp (8 significant bits) of the larger magnitude: x = m 2^e, 0.5 <= m < 1 -> ulp = 2^(e - 8)
    big = torch.maximum(f0.abs(), want.abs())
    ulp = torch.ldexp(torch.ones_like(big), torch.frexp(big).exponent - 8)
    diff = (f0 - want).abs()
    print(f"z0 factor: {int((diff > 0).sum())} of {diff.numel()} elements differ, worst {float((diff / ulp).max()):.2f} ulp")
    assert (diff <= ulp).all()


def _forward(eng, gb, z_init):
    eng.z_init = z_init
    before = eng.z_forwards
    h, e = eng.forward(gb)
    torch.cuda.synchronize()
    ws = eng.workspace(gb.num_nodes, gb.num_edges)
    return (h, e, eng.last_hT.clone(), ws["alpha"].clone()), eng.z_forwards - before


@pytest.fixture(scope="module")
def gb2():
    return _batch([40, 55, 21, 64])  # two complexes


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [2, 4])
def test_engine_z_init_bit_identical(gb2, layers):
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.engine import GeoTEngine
    from deepinteract_amd.weights import seeded_state_dict
    cfg = GeoTConfig(num_gnn_layers=layers)
    e = GeoTEngine(seeded_state_dict(0, cfg, with_head=False), "bf16", cfg)
    ref, nz = _forward(e, gb2, False)
    assert nz == 0
    got, nz = _forward(e, gb2, True)
    assert nz == 1
    for a, b, what in zip(ref, got, ("node feats", "edge feats", "last_hT", "alpha")):
        assert torch.isfinite(a.float()).all(), what
        assert torch.equal(a, b), what


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_layer", "fp32", "no_geo_ref", "fold_attn"])
def test_engine_keeps_the_f_path(gb2, case):
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.engine import GeoTEngine
    from deepinteract_amd.weights import seeded_state_dict
    cfg = GeoTConfig(num_gnn_layers=1 if case == "one_layer" else 2)
    e = GeoTEngine(seeded_state_dict(0, cfg, with_head=False), "f32" if case == "fp32" else "bf16", cfg)
    e.fold_attn = case == "fold_attn"
    gb = gb2.with_geo_ref(False) if case == "no_geo_ref" else gb2
    ref, nz0 = _forward(e, gb, False)
    got, nz1 = _forward(e, gb, True)
    assert nz0 == 0 and nz1 == 0
    outs = ("node feats", "edge feats", "last_hT") + (() if case == "fold_attn" else ("alpha",))  # the fold writes no alpha
    for a, b, what in zip(ref, got, outs):
        assert torch.isfinite(a.float()).all(), what
        assert torch.equal(a, b), what


def test_entry_points_refuse_bad_arguments():
    """Host-side returns before any launch (dummy non-NULL pointers are never dereferenced)."""
    from deepinteract_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    ref = _lib.DiGraph(8, 16, 16, 16, 16, 16, 16, _lib.DI_GRAPH_GEO_REF)
    plain = _lib.DiGraph(8, 16, 16, 16, 16, 16, 16, 0)

    def init(g, dt, init_wmat=p, z=p):
        return lib.di_embed_init_edge_z(ctypes.byref(g), dt, 113, p, p, p, p, p, p, init_wmat, p, p, p, z, None, -1, None)

    def layer(g, dt, z=p, init_wmat=p):
        return lib.di_edge_layer_z(ctypes.byref(g), dt, p, z, init_wmat, p, p, p, p, p, None)

    for fn in (init, layer):
        assert fn(ref, _lib.DI_F32) == -1
        assert fn(plain, _lib.DI_BF16) == -1
        assert fn(ref, _lib.DI_BF16, z=None) == -1
        assert fn(ref, _lib.DI_BF16, init_wmat=None) == -1
