"""Contact-head benchmark (outside the metric): the regional attention block (use_interact_attention) on HIP
against the module's plain-torch path, alone and inside the whole head. Seeded weights of the attention
configuration; the block's input is a normal sample [1, 128, side, side].

Per side (64, 256, 1000) and dtype (bf16, fp32):
  block   scores, v and mix timed one by one and together (HeadAttnOps; v is di_head_conv for bf16 --
          cin = cout = 128, no bias -- and torch's 1x1 convolution for fp32), against
          MultiHeadRegionalAttention.forward (torch, nine shifted views) and, where memory allows, against
          the reference's formulation restated in torch: q, k and v stretched ninefold by the one-hot
          Conv3d, a softmax over the stretched scores, a [9, 128, H, W] product and its sum.
          ``mix_bytes`` = v + scores + y, what the mix has to move; ``mix_TBps`` = that over its time, to
          read against the 6.0 TB/s plain-store figure of DESIGN.md section 8.
  head    the whole head (HIP norm passes; bf16: HIP convolutions) with and without the option, and the
          time the option adds.
Method of tools/bench_head_batch.py: HIP events on one stream, every case warmed up, sides timed in
alternating windows of ``--reps`` calls, the median window reported with the fastest and slowest.
Needs a GPU: there is no CPU path.

usage: python tools/bench_head_attn.py [--reps 3] [--windows 5] [--sides 64,256,1000] [--no-head]
                                       [--out profiles/head_attn_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_head_batch import window  # noqa: E402
from deepinteract_amd.config import GeoTConfig  # noqa: E402
from deepinteract_amd.head import HeadConvOps, HeadNormOps, ResNet2DInputWithOptAttention  # noqa: E402
from deepinteract_amd.weights import seeded_state_dict  # noqa: E402

PLAIN_STORE_TBPS = 6.0


def head(dtype, attention):
    sd = seeded_state_dict(0, GeoTConfig(use_interact_attention=attention))
    hsd = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
    m = ResNet2DInputWithOptAttention(use_attention=attention).cuda().eval()
    m.load_state_dict(hsd)
    m = m.to(dtype=dtype).use_hip_norm_ops(HeadNormOps("cuda"))
    return m.use_hip_convs(HeadConvOps("cuda")) if dtype == torch.bfloat16 else m


def stretched_form(mha, x):
    """The block as the reference formulates it: every one of q, k, v copied into nine shifted planes by
    the one-hot Conv3d, then softmax, product and sum over the nine."""
    B, _, H, W = x.shape
    w = mha.stretch_layer.weight
    q, k, v = (F.conv3d(layer(x)[:, None], w, padding=(0, 1, 1)) for layer in (mha.q_layer, mha.k_layer, mha.v_layer))
    s = (q * k).view(B, 9, mha.n_head, mha.dk_per_head, H, W).sum(3) / mha.temper
    att = torch.softmax(s, 1)
    return (att[:, :, :, None] * v.view(B, 9, mha.n_head, mha.dv_per_head, H, W)).sum(1).view(B, -1, H, W)


def timed(fns, reps, windows):
    """name -> (median, min, max) ms per call; the sides alternate window by window."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(window(fn, reps))
    return {k: [statistics.median(v), min(v), max(v)] for k, v in t.items()}


def block_case(m, side, dtype, reps, windows):
    mha, aops, cops = m.MHA2D_1, m.aops, m.cops
    g = torch.Generator(device="cuda").manual_seed(side)
    x = torch.randn(1, 128, side, side, generator=g, device="cuda").to(dtype)
    wq, wk = m._qk(mha)
    es = x.element_size()
    y = torch.empty_like(x)

    def value():
        return cops.conv(x, mha.v_layer.weight, in_elu=False) if cops is not None else mha.v_layer(x)

    s, v = aops.scores(x, wq, wk), value()
    fns = {"scores": lambda: aops.scores(x, wq, wk, out=s), "v": value, "mix": lambda: aops.mix(v, s, out=y),
           "hip_block": lambda: aops.mix(value(), aops.scores(x, wq, wk, out=s), out=y),
           "torch_block": lambda: mha(x)[0]}
    row = {"shape": [side, side], "dtype": str(dtype).split(".")[-1]}
    try:
        ref = stretched_form(mha, x)
        fns["stretched_torch"] = lambda: stretched_form(mha, x)
    except torch.cuda.OutOfMemoryError:
        ref = None
        row["stretched_torch"] = "not run: out of memory"
    got, tor = fns["hip_block"]().float(), fns["torch_block"]().float()
    row["max_abs_diff_hip_vs_torch"] = float((got - tor).abs().max())
    if ref is not None:
        row["max_abs_diff_torch_vs_stretched"] = float((tor - ref.float()).abs().max())
    del ref
    torch.cuda.empty_cache()
    row["ms"] = timed(fns, reps, windows)
    px = side * side
    row["mix_bytes"] = px * (128 * es * 2 + 4 * 4)
    row["mix_TBps"] = row["mix_bytes"] / (row["ms"]["mix"][0] * 1e-3) / 1e12
    row["mix_share_of_plain_store"] = row["mix_TBps"] / PLAIN_STORE_TBPS
    row["scores_bytes"] = px * (128 * es + 4 * 4)
    row["scores_gflop"] = px * 128 * 32 * 2 / 1e9
    row["torch_over_hip"] = row["ms"]["torch_block"][0] / row["ms"]["hip_block"][0]
    return row


def head_case(heads, side, dtype, reps, windows):
    g = torch.Generator(device="cuda").manual_seed(side + 1)
    t = torch.randn(1, 256, side, side, generator=g, device="cuda").to(dtype)
    ms = timed({"with_attention": lambda: heads[True](t), "without": lambda: heads[False](t)}, reps, windows)
    return {"shape": [side, side], "dtype": str(dtype).split(".")[-1], "ms": ms,
            "attention_adds_ms": ms["with_attention"][0] - ms["without"][0],
            "attention_adds_share": ms["with_attention"][0] / ms["without"][0] - 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sides", default="64,256,1000")
    ap.add_argument("--no-head", action="store_true", help="the block alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_attn_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_attn needs a ROCm GPU")
    sides = [int(s) for s in a.sides.split(",")]
    blocks, heads_rows = [], []
    with torch.no_grad():
        for dtype in (torch.bfloat16, torch.float32):
            heads = {att: head(dtype, att) for att in (True, False)}
            for side in sides:
                blocks.append(block_case(heads[True], side, dtype, a.reps, a.windows))
                print(json.dumps(blocks[-1]), flush=True)
                if not a.no_head:
                    heads_rows.append(head_case(heads, side, dtype, max(1, a.reps // 2), a.windows))
                    print(json.dumps(heads_rows[-1]), flush=True)
                torch.cuda.empty_cache()
    out = {"workload": "the contact head's regional attention block (scores, value convolution, 3x3 softmax mix) on "
                       "one [1, 128, side, side] image, and the whole head (58 + 4 blocks) with and without it",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "timing": "HIP events on the current stream, alternating windows; [median, min, max] ms per call",
           "plain_store_TBps": PLAIN_STORE_TBPS, "block": blocks, "head": heads_rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
