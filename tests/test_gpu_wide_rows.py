"""The 32x32 bf16 kernels' 16-B row accesses (csrc/mfma32.h: R32::load + unswz, store_row32) against
the ``rows8`` build (DI_ROW_WIDE=0: the same rows as 8-B accesses; tools/build_variants.py, built by
__graft_entry__.build()). The change is data movement only, so every output is compared bit for bit.

One child process binds the product library and one the variant (deepinteract_amd._lib.load_variant,
the pattern of tests/test_gpu_variants.py); each runs the same seeded inputs once and returns every
output, and the tests compare the two sets.

Graphs (device builder, bf16, seeded_state_dict(0)) -- the smallest edge counts at which a wave's
row clamp, a partial wave and a second 256-edge tile are exercised:
  * k = 3, one chain of 7: 21 edges, less than one wave, lane pairs 21..31 clamped to the last row;
  * k = 3, one chain of 11: 33 edges, one full wave plus one row;
  * k = 20, chains [20, 21]: 820 edges, four 256-edge tiles with a ragged last one, two chains.
Engine configurations, each on each graph:
  * default: z path, 2 layers, DI_GRAPH_GEO_REF (k_init_x32<true, true>, k_edge_x32_ring<0, true, true>
    and <1, true, false>);
  * z_init off: the F form of InitEdge and layer 0 (<0, true, false>);
  * 3 layers: <0, true, false> as a middle layer;
  * with_geo_ref(False): the general path, the gathered xn rows and the fn store (k_init_x32<false>,
    k_edge_x32_ring<*, false, false>);
  * fold_attn: the fold's V row.
And di_edge_layer (non-final and final) through the ctypes entry points on f_in / qkv / f_out views
that start 8 bytes into their buffers: rows that are 8-B but not 16-B aligned.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS8 = os.path.join(ROOT, "deepinteract_amd", "lib", "variants", "rows8", "libdeepinteract_amd.so")

# name -> (chain sizes, k, expected edge count)
GRAPHS = {"e21_under_one_wave": ([7], 3, 21), "e33_wave_plus_one_row": ([11], 3, 33),
          "e820_four_tiles_ragged": ([20, 21], 20, 820)}
CONFIGS = ("default", "f_form", "three_layers", "general", "fold")


def _bits(t):
    """A tensor's bit pattern as a numpy array (bf16 -> int16): crosses the process boundary as is."""
    t = t.detach().contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _engine_outputs(out, sd_of, gbs):
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.engine import GeoTEngine
    for cfg_name in CONFIGS:
        cfg = GeoTConfig(num_gnn_layers=3 if cfg_name == "three_layers" else 2)
        eng = GeoTEngine(sd_of(cfg), "bf16", cfg)
        eng.z_init = cfg_name not in ("f_form",)
        eng.fold_attn = cfg_name == "fold"
        for gname, gb in gbs.items():
            g = gb.with_geo_ref(False) if cfg_name == "general" else gb
            before = eng.z_forwards
            h, e = eng.forward(g)
            torch.cuda.synchronize()
            took_z = eng.z_forwards - before
            assert took_z == (1 if cfg_name in ("default", "three_layers") else 0), (cfg_name, gname, took_z)
            res = {"h": _bits(h), "edge": _bits(e), "hT": _bits(eng.last_hT)}
            if cfg_name != "fold":  # the fold writes no alpha
                res["alpha"] = _bits(eng.workspace(g.num_nodes, g.num_edges)["alpha"])
            out[f"{cfg_name}/{gname}"] = res


def _offset_view(n_rows, width, fill=None, src=None):
    """A [n_rows, width] bf16 view starting 4 elements (8 bytes) into its buffer."""
    buf = torch.full((n_rows * width + 8,), float("nan") if fill is None else fill, dtype=torch.bfloat16, device="cuda")
    v = buf[4:4 + n_rows * width].view(n_rows, width)
    assert v.data_ptr() % 16 == 8
    if src is not None:
        v.copy_(src)
    return buf, v


def _edge_layer_offset_rows(out, sd, gb):
    """di_edge_layer, non-final then final, on rows 8 bytes off 16-B alignment."""
    from deepinteract_amd import _lib
    from deepinteract_amd.engine import GeoTEngine
    eng = GeoTEngine(sd, "bf16")
    lib, p = eng.lib, eng.packed
    nt, et = gb.num_nodes, gb.num_edges
    gen = torch.Generator().manual_seed(1234)
    keep = []

    def rows(n, w):
        buf, v = _offset_view(n, w, src=(0.5 * torch.randn(n, w, generator=gen)).bfloat16().cuda())
        keep.append(buf)
        return v

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    f_in, qkv = rows(et, 128), rows(nt, 384)
    g = ctypes.byref(gb.c_graph)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for final in (0, 1):
        em, ev = p.edge[final]
        alpha = torch.full((et, 4), float("nan"), device="cuda")
        buf, f_out = _offset_view(et, 128)
        rc = lib.di_edge_layer(g, _lib.DI_BF16, final, ptr(gb.edge_f), ptr(f_in), None, ptr(qkv), ptr(em), ptr(ev),
                               ptr(alpha), None if final else ptr(f_out), None, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        res = {"alpha": _bits(alpha)}
        if not final:
            res["f_out"] = _bits(f_out)
            # nothing written outside the rows
            assert torch.isnan(buf[:4].float()).all() and torch.isnan(buf[4 + et * 128:].float()).all()
        out[f"offset_rows/{'final' if final else 'layer'}"] = res


def _child(variant, q):
    try:
        from deepinteract_amd import _lib
        if variant:
            _lib.load_variant(variant)
        from deepinteract_amd import synth
        from deepinteract_amd.builder import build_graph_batch
        from deepinteract_amd.weights import seeded_state_dict
        gbs = {}
        for name, (sizes, k, et) in GRAPHS.items():
            chains = [synth.synthetic_chain(n, 8100 + i) for i, n in enumerate(sizes)]
            gb = build_graph_batch(chains, k=k, nbr_seeds=list(range(1, len(sizes) + 1)))
            assert gb.num_edges == et and gb.geo_ref, (name, gb.num_edges, gb.geo_ref)
            gbs[name] = gb
        sds = {}

        def sd_of(cfg):
            if cfg.num_gnn_layers not in sds:
                sds[cfg.num_gnn_layers] = seeded_state_dict(0, cfg, with_head=False)
            return sds[cfg.num_gnn_layers]

        out = {}
        _engine_outputs(out, sd_of, gbs)
        from deepinteract_amd.config import GeoTConfig
        _edge_layer_offset_rows(out, sd_of(GeoTConfig(num_gnn_layers=2)), gbs["e820_four_tiles_ragged"])
        q.put((out, None))
    except Exception as exc:
        import traceback
        q.put((None, f"{exc!r}\n{traceback.format_exc()}"))


def _run(variant):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(variant, q))
    p.start()
    try:
        out, err = q.get(timeout=240)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert p.exitcode == 0
    return out


@pytest.fixture(scope="module")
def both():
    """(product outputs, rows8 outputs), each computed once in its own process."""
    assert os.path.exists(ROWS8), "variant rows8 not built: python tools/build_variants.py rows8"
    return _run(None), _run(ROWS8)


def _same(both, key):
    wide, narrow = both[0][key], both[1][key]
    assert sorted(wide) == sorted(narrow)
    for what in sorted(wide):
        a, b = torch.from_numpy(wide[what]), torch.from_numpy(narrow[what])
        vals = a.view(torch.bfloat16).float() if a.dtype == torch.int16 else a
        assert torch.isfinite(vals).all(), (key, what)
        assert torch.equal(a, b), (key, what, int((a != b).sum()))


@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("config", CONFIGS)
def test_engine_outputs_bit_identical(both, config, graph):
    _same(both, f"{config}/{graph}")


@pytest.mark.parametrize("which", ["layer", "final"])
def test_edge_layer_on_rows_8_bytes_off_alignment(both, which):
    _same(both, f"offset_rows/{which}")
