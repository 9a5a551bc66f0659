"""Generate tests/golden/sat_tiny.npz: the reference's own LitGINI, unmodified, through refshim, with
weights under which both attention clamps (graph_utils.py:29-32, :58-61) bind -- the fixture that pins
WHERE the reference clamps, which tiny.npz / plain_tiny.npz cannot (no value of theirs reaches +-5).
Runs only where the reference project is present (refshim.REFERENCE_ROOT).

Two models of two layers, loaded strictly:
  geo    ``seeded_state_dict(0)`` with tests/geot_cases.py's SAT_FACTORS applied;
  plain  ``seeded_state_dict(plain_cases.SAT_SEED, GeoTConfig(disable_geometric_mode=True))`` with
         tests/plain_cases.py's factors for a two-layer model.
Input: ``synth.synthetic_complex(9, 33, 21)``, graph seeds 101 / 102 (plain_tiny.npz's complex: 660 and
420 edges).

Stored: each chain's graph arrays once (``g1_*``, ``g2_*``); per mode, under ``<mode>_``, what
plain_tiny.npz stores under the same names: ``init_edge``, the layer-0 node / edge outputs, the final
node outputs and the last intermediate layer's edges, logits, the weights' SHA-256 and the factors
(``<mode>_factors``: rows of gt_block, s_qk, s_p). The [E, 128] edge stages are sampled rows (each with
the chain's last row) plus float64 column sums over all rows.

Usage:  python tests/golden/make_golden_saturated.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)

import refshim  # noqa: E402
from make_golden import KNN, ref_graph  # noqa: E402
from make_golden_plain import _rows  # noqa: E402
import geot_cases as C  # noqa: E402
import plain_cases as P  # noqa: E402
from deepinteract_amd import synth  # noqa: E402
from deepinteract_amd.config import GeoTConfig  # noqa: E402
from deepinteract_amd.weights import seeded_state_dict, state_dict_sha256  # noqa: E402

SEEDS = (101, 102)
LAYERS = 2


def weights(mode):
    """(state dict with the head, {gt_block: (s_qk, s_p)}) of one mode."""
    if mode == "geo":
        factors = {li: C.SAT_FACTORS[li] for li in range(LAYERS)}
        return C.scale_attention(seeded_state_dict(0), factors), factors
    factors = P.block_factors(LAYERS)
    return C.scale_attention(seeded_state_dict(P.SAT_SEED, GeoTConfig(disable_geometric_mode=True)), factors), factors


def main():
    import torch.nn as nn
    dm, du = refshim.reference_modules()
    dgl = sys.modules["dgl"]
    ch1, ch2 = synth.synthetic_complex(9, 33, 21)
    g1, g2 = ref_graph(du, ch1, SEEDS[0]), ref_graph(du, ch2, SEEDS[1])
    out = {}
    for tag, g, ch, seed in (("g1", g1, ch1, SEEDS[0]), ("g2", g2, ch2, SEEDS[1])):
        src, dst = g.edges()
        out[f"{tag}_backbone"], out[f"{tag}_amide_norm"], out[f"{tag}_dips"] = ch["backbone"], ch["amide_norm"], ch["dips"]
        out[f"{tag}_src"], out[f"{tag}_dst"] = src.numpy().astype(np.int32), dst.numpy().astype(np.int32)
        out[f"{tag}_node_f"] = g.ndata["f"].numpy().astype(np.float32)
        out[f"{tag}_edge_f"] = g.edata["f"].numpy().astype(np.float32)
        out[f"{tag}_src_nbr"] = g.edata["src_nbr_e_ids"].numpy().astype(np.int32)
        out[f"{tag}_dst_nbr"] = g.edata["dst_nbr_e_ids"].numpy().astype(np.int32)
        out[f"{tag}_nbr_seed"] = np.array(seed)
        assert src.numel() == g.num_nodes() * KNN

    for mode in ("geo", "plain"):
        model = dm.LitGINI(num_node_input_feats=113, num_edge_input_feats=27, gnn_activ_fn=nn.SiLU(), num_classes=2,
                           num_gnn_layers=LAYERS, num_interact_layers=14, dropout_rate=0.2, use_wandb_logger=False,
                           disable_geometric_mode=mode == "plain")
        sd, factors = weights(mode)
        model.load_state_dict(sd, strict=True)
        model.eval()
        out[f"{mode}_weights_sha256"] = np.array(state_dict_sha256(sd))
        out[f"{mode}_factors"] = np.array([[li, *factors[li]] for li in sorted(factors)], dtype=np.float64)
        rec = {}

        def hook(name):
            def fn(mod, inp, outp):
                rec.setdefault(name, []).append(outp)
            return fn

        gm = model.gnn_module[0]
        hs = [gm.init_edge_module.register_forward_hook(hook("init_edge")),
              gm.gt_block[0].register_forward_hook(hook("layer0"))]
        with torch.no_grad():
            logits_list, n1, e1, n2, e2 = model.shared_step(dgl.batch([g1]), dgl.batch([g2]), return_representations=True)
        for h in hs:
            h.remove()
        out[f"{mode}_logits"] = logits_list[0].numpy().astype(np.float32)

        def sampled(tag, name, full, every):
            full = np.asarray(full)
            rows = _rows(full.shape[0], every)
            out[f"{mode}_{tag}_{name}_rows"] = rows
            out[f"{mode}_{tag}_{name}"] = full[rows].astype(np.float32)
            out[f"{mode}_{tag}_{name}_colsum"] = full.astype(np.float64).sum(0)

        for ci, (tag, n, e) in enumerate((("g1", n1, e1), ("g2", n2, e2))):
            out[f"{mode}_{tag}_node_out"] = np.asarray(n).astype(np.float32)
            sampled(tag, "edge_out", e, 4)
            out[f"{mode}_{tag}_edge_rows"] = out.pop(f"{mode}_{tag}_edge_out_rows")  # tiny.npz's name
            sampled(tag, "init_edge", rec["init_edge"][ci].numpy(), 4)
            out[f"{mode}_{tag}_layer0_node"] = rec["layer0"][ci][0].numpy().astype(np.float32)
            sampled(tag, "layer0_edge", rec["layer0"][ci][1].numpy(), 4)
    path = os.path.join(HERE, "sat_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB", out["geo_logits"].shape)


if __name__ == "__main__":
    main()
