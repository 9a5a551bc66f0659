"""Generate tests/golden/plain_tiny.npz: the reference's own LitGINI with disable_geometric_mode=True
(the plain Graph Transformer baseline), unmodified, through refshim -- as make_golden.py does for the
geometric mode. Runs only where the reference project is present (refshim.REFERENCE_ROOT).

Weights: ``seeded_state_dict(0, GeoTConfig(disable_geometric_mode=True))`` loaded strictly (its
SHA-256 is stored). Input: ``synth.synthetic_complex(9, 33, 21)``, graph seeds 101 / 102: 660 and 420
edges, neither a multiple of the kernels' 64-row tile.

Stored, named as tiny.npz names them: each chain's graph arrays; ``init_edge`` and the layer-0 node /
edge outputs (forward hooks); the final node outputs; logits and probabilities; the GeoT key names and
shapes. The [E, 128] edge stages are stored as sampled rows (``g*_init_edge_rows``,
``g*_layer0_edge_rows``, ``g*_edge_rows``, each with the chain's last row) plus float64 column sums
over ALL rows, which keeps the file well under the repository's size limit.

Usage:  python tests/golden/make_golden_plain.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import refshim  # noqa: E402
from make_golden import KNN, ref_graph  # noqa: E402
from deepinteract_amd import synth  # noqa: E402
from deepinteract_amd.config import GeoTConfig  # noqa: E402
from deepinteract_amd.weights import geot_keys, seeded_state_dict, state_dict_sha256  # noqa: E402

WEIGHT_SEED = 0
SEEDS = (101, 102)


def _rows(n, every):
    r = np.arange(0, n, every)
    return (r if r[-1] == n - 1 else np.append(r, n - 1)).astype(np.int32)


def main():
    import torch.nn as nn
    dm, du = refshim.reference_modules()
    dgl = sys.modules["dgl"]
    cfg = GeoTConfig(disable_geometric_mode=True)
    model = dm.LitGINI(num_node_input_feats=113, num_edge_input_feats=27, gnn_activ_fn=nn.SiLU(), num_classes=2,
                       num_gnn_layers=2, num_interact_layers=14, dropout_rate=0.2, use_wandb_logger=False,
                       disable_geometric_mode=True)
    sd = seeded_state_dict(WEIGHT_SEED, cfg)
    model.load_state_dict(sd, strict=True)
    model.eval()
    out = {"weights_sha256": np.array(state_dict_sha256(sd))}
    ref_sd = model.state_dict()
    names = [k for k, _, _ in geot_keys(cfg)]
    assert sorted(names) == sorted(k for k in ref_sd if not k.startswith("interact_module.")), "GeoT key set"
    out["geot_key_names"] = np.array(names)
    out["geot_key_shapes"] = np.array([",".join(str(d) for d in ref_sd[k].shape) for k in names])

    ch1, ch2 = synth.synthetic_complex(9, 33, 21)
    g1, g2 = ref_graph(du, ch1, SEEDS[0]), ref_graph(du, ch2, SEEDS[1])
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

    rec = {}

    def hook(name):
        def fn(mod, inp, outp):
            rec.setdefault(name, []).append(outp)
        return fn

    gm = model.gnn_module[0]
    assert isinstance(gm.init_edge_module, nn.Linear) and isinstance(gm.gt_block[1].conformation_module, nn.Linear)
    hs = [gm.init_edge_module.register_forward_hook(hook("init_edge")),
          gm.gt_block[0].register_forward_hook(hook("layer0"))]
    with torch.no_grad():
        logits_list, n1, e1, n2, e2 = model.shared_step(dgl.batch([g1]), dgl.batch([g2]), return_representations=True)
    for h in hs:
        h.remove()
    logits = logits_list[0]
    L1, L2 = logits.shape[-2:]
    flat = torch.flatten(logits.squeeze(0), start_dim=1).transpose(1, 0)  # lit_model_predict.py:236-239
    out["logits"] = logits.numpy().astype(np.float32)
    out["probs"] = torch.softmax(flat, dim=1)[:, 1].reshape(L1, L2).numpy().astype(np.float32)

    def sampled(tag, name, full, every):
        full = np.asarray(full)
        rows = _rows(full.shape[0], every)
        out[f"{tag}_{name}_rows"] = rows
        out[f"{tag}_{name}"] = full[rows].astype(np.float32)
        out[f"{tag}_{name}_colsum"] = full.astype(np.float64).sum(0)

    for ci, (tag, n, e) in enumerate((("g1", n1, e1), ("g2", n2, e2))):
        out[f"{tag}_node_out"] = np.asarray(n).astype(np.float32)
        sampled(tag, "edge_out", e, 4)
        out[f"{tag}_edge_rows"] = out.pop(f"{tag}_edge_out_rows")  # tiny.npz's name
        sampled(tag, "init_edge", rec["init_edge"][ci].numpy(), 2)
        out[f"{tag}_layer0_node"] = rec["layer0"][ci][0].numpy().astype(np.float32)
        sampled(tag, "layer0_edge", rec["layer0"][ci][1].numpy(), 2)
    path = os.path.join(HERE, "plain_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB", out["logits"].shape, len(names), "GeoT keys")


if __name__ == "__main__":
    main()
