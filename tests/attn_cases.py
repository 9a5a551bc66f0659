"""The head's regional attention restated in float64 (the reference of tests/test_head_attn_host.py and
tests/test_gpu_head_attn.py), the fixture it is pinned to, and the shapes both suites share.

The restatement follows MultiHeadRegionalAttention (deepinteract_modules.py:1109-1152) as the head builds
it (128 channels, 4 heads, d_k 16, region 3), without its ninefold stretch:
  q = Wq a, k = Wk a, v = Wv a per pixel;  s[h, p] = 1/4 sum_{j = 4h .. 4h+3} q[j, p] k[j, p];
  out[c, p] = sum over the 9 taps d of softmax_d(s[c // 32, p + d]) v[c, p + d],
a tap outside the image counting with score 0 and value 0 and staying in the softmax's denominator.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAPS = [(i, j) for i in range(3) for j in range(3)]

# 1x1, strips, an odd plane (17x33: planes on 2-B / 4-B boundaries), more than one block, and one pixel
# count on each side of every edge the kernels have: 4 and 8 pixels per lane (3x5 = 15, 4x4 = 16, 17x1),
# the scores' 1024-pixel tile (32x32, 1025 = 25x41, 1028 = 4x257), the mix's 2048-pixel run (32x64,
# 2056 = 8x257, 33x65) and 256-pixel element block (16x16, 257x1)
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (4, 4), (17, 1), (16, 16), (257, 1), (17, 33), (32, 32), (25, 41),
          (4, 257), (32, 64), (8, 257), (33, 65), (145, 145)]


def scores64(a, wq, wk):
    """a [128, H, W], wq / wk [16, 128], all float64 -> s [4, H, W]."""
    q = torch.einsum("oc,chw->ohw", wq, a)
    k = torch.einsum("oc,chw->ohw", wk, a)
    return (q * k).view(4, 4, *a.shape[1:]).sum(1) / 4.0


def weights64(s):
    """s [4, H, W] -> the attention weights [9, 4, H, W]: softmax over the taps, outside taps at score 0."""
    H, W = s.shape[1:]
    sp = F.pad(s, (1, 1, 1, 1))
    return torch.softmax(torch.stack([sp[:, i:i + H, j:j + W] for i, j in TAPS]), 0)


def mix64(v, s):
    """v [128, H, W], s [4, H, W] float64 -> out [128, H, W]."""
    H, W = s.shape[1:]
    A = weights64(s)
    vp = F.pad(v, (1, 1, 1, 1))
    return sum(A[n].repeat_interleave(32, 0) * vp[:, i:i + H, j:j + W] for n, (i, j) in enumerate(TAPS))


def restate(x, wq, wk, wv):
    """The whole block in float64: x [128, H, W] -> (out [128, H, W], attention weights [4, 9, H, W])."""
    x, wq, wk, wv = (t.double() for t in (x, wq, wk, wv))
    s = scores64(x, wq, wk)
    v = torch.einsum("oc,chw->ohw", wv, x)
    return mix64(v, s), weights64(s).permute(1, 0, 2, 3)


def scores_bound(a, wq, wk):
    """The fp32 scores' error bound per pixel and head, [4, H, W] float64:
    (2 * 131 * 2^-24 + 4e-6) * 1/4 sum_j (sum_c |wq_jc a_c|)(sum_c |wk_jc a_c|): two 128-term fp32 dot
    products (and the 4-term sum and the scaling) and the ELU's 1e-6 on each factor."""
    aq = torch.einsum("oc,chw->ohw", wq.abs(), a.abs())
    ak = torch.einsum("oc,chw->ohw", wk.abs(), a.abs())
    return (2 * 131 * 2.0 ** -24 + 4e-6) * (aq * ak).view(4, 4, *a.shape[1:]).sum(1) / 4.0


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/attn_head.npz (the reference's own head with use_attention=True, CPU fp32) as tensors."""
    z = np.load(os.path.join(GOLDEN, "attn_head.npz"))
    return {k: (str(z[k]) if z[k].dtype.kind == "U" else torch.as_tensor(z[k])) for k in z.files}


@functools.lru_cache(maxsize=None)
def attention_state_dict():
    from deepinteract_amd.config import GeoTConfig
    from deepinteract_amd.weights import seeded_state_dict
    return seeded_state_dict(0, GeoTConfig(use_interact_attention=True))


def head_state_dict():
    p = "interact_module."
    return {k[len(p):]: v for k, v in attention_state_dict().items() if k.startswith(p)}


def block_weights(i):
    """(wq [16, 128], wk [16, 128], wv [128, 128]) fp32 of MHA2D_i."""
    sd = head_state_dict()
    return tuple(sd[f"MHA2D_{i}.{n}_layer.weight"][:, :, 0, 0] for n in "qkv")


def build_head(dtype=torch.float32):
    """This project's head with attention, the fixture's weights loaded, eval mode, on the CPU."""
    from deepinteract_amd.head import ResNet2DInputWithOptAttention
    head = ResNet2DInputWithOptAttention(14, 256, 128, 2, use_attention=True).eval()
    head.load_state_dict(head_state_dict())
    return head.to(dtype)
