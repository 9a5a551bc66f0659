"""Generate tests/golden/attn_head.npz from the REFERENCE's own contact head with regional attention.

Runs only where the reference checkout is present (``refshim`` locates it and is used as it is). The reference's
``ResNet2DInputWithOptAttention(num_chunks=14, init_channels=256, use_attention=True)``
(deepinteract_modules.py:1155-1248, MultiHeadRegionalAttention :1109-1152) runs unmodified on the CPU
in fp32, in eval mode, on a seeded normal [1, 256, 11, 19] input.

Weights: the ``interact_module.*`` tensors of ``seeded_state_dict(0)`` for the attention configuration
(``GeoTConfig(use_interact_attention=True)``), loaded with a strict ``load_state_dict``; the SHA-256 of
the whole seeded state dict is stored so drift is caught.

Stored: the input, the logits, and per attention block (MHA2D_1, MHA2D_2) its input, its output and its
attention scores [4, 9, H, W], taken by forward hooks.

Usage:  python tests/golden/make_golden_attention.py
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
from deepinteract_amd.config import GeoTConfig  # noqa: E402
from deepinteract_amd.weights import seeded_state_dict, state_dict_sha256  # noqa: E402

WEIGHT_SEED, INPUT_SEED = 0, 0
H, W = 11, 19


def main():
    dm, _ = refshim.reference_modules()
    sd = seeded_state_dict(WEIGHT_SEED, GeoTConfig(use_interact_attention=True))
    p = "interact_module."
    head = dm.ResNet2DInputWithOptAttention(num_chunks=14, init_channels=256, num_channels=128, num_classes=2,
                                            use_attention=True).eval()
    head.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
    x = torch.randn(1, 256, H, W, generator=torch.Generator().manual_seed(INPUT_SEED))
    rec = {}
    for name in ("MHA2D_1", "MHA2D_2"):
        def hook(_m, inp, out, name=name):
            rec[name] = (inp[0].detach(), out[0].detach(), out[1].detach())
        head._modules[name].register_forward_hook(hook)
    with torch.no_grad():
        logits = head(x)
    out = {"input": x.numpy(), "logits": logits.numpy(), "weights_sha256": np.array(state_dict_sha256(sd)),
           "weight_seed": np.array(WEIGHT_SEED)}
    for i, name in enumerate(("MHA2D_1", "MHA2D_2"), 1):
        a, o, s = rec[name]
        out[f"block{i}_in"], out[f"block{i}_out"], out[f"block{i}_scores"] = a.numpy(), o.numpy(), s.numpy()
        print(name, "in absmax", float(a.abs().max()), "out absmax", float(o.abs().max()),
              "scores", tuple(s.shape))
    path = os.path.join(HERE, "attn_head.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; logits absmax", float(logits.abs().max()))


if __name__ == "__main__":
    main()
