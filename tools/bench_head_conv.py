"""Per-launch times of the head convolutions (head.HeadConvOps: csrc/head_conv.hip in bf16,
csrc/head_conv_f32.hip in fp32) on one [C, L, L] image, beside torch's convolution (MIOpen) of the same
shape and dtype: each convolution the head uses, with the fused transform + statistics (``hip_fused``) and
without (``hip_plain``), then the block-input statistics pass and the fold. Prints one JSON line (outside
the metric); the fp32 rows also carry the plain launch's TFLOP/s (the f32-input MFMA peaks at 155).

usage: python tools/bench_head_conv.py [L=1000] [bf16|f32]
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepinteract_amd.head import HeadConvOps  # noqa: E402

SHAPES = ((128, 64, 1, 1), (64, 64, 3, 1), (64, 64, 3, 2), (64, 64, 3, 4), (64, 64, 3, 8), (64, 128, 1, 1),
          (128, 128, 1, 1))  # cin, cout, ksize, dilation


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}[sys.argv[2] if len(sys.argv) > 2 else "bf16"]
    cops = HeadConvOps("cuda")
    out = {"L": L, "dtype": str(dt).split(".")[-1]}
    for cin, cout, k, d in SHAPES:
        x = torch.randn(1, cin, L, L, device="cuda").to(dt)
        w = (torch.randn(cout, cin, k, k, device="cuda") / (cin * k * k) ** 0.5).to(dt)
        s = torch.rand(cin, device="cuda") + 0.5
        b = torch.randn(cin, device="cuda")
        t_hip = timed(lambda: cops.conv(x, w, in_scale=s, in_shift=b, in_elu=True, dilation=d, stats=True))
        t_plain = timed(lambda: cops.conv(x, w, dilation=d))
        t_mi = timed(lambda: F.conv2d(x, w, None, 1, d if k == 3 else 0, d))
        gb = (cin + cout) * L * L * x.element_size() / 1e9  # one read of the input, one write of the output
        rec = {"hip_fused_ms": round(t_hip, 4), "hip_plain_ms": round(t_plain, 4),
               "miopen_ms": round(t_mi, 4), "hip_fused_GBps": round(gb / t_hip * 1e3, 1)}
        if dt == torch.float32:
            tf = 2.0 * cin * cout * k * k * L * L / 1e9
            rec["hip_fused_tflops"], rec["hip_plain_tflops"] = round(tf / t_hip, 1), round(tf / t_plain, 1)
        out[f"{cin}to{cout}_k{k}_d{d}"] = rec
    x = torch.randn(1, 128, L, L, device="cuda").to(dt)
    out["plane_stats_128_ms"] = round(timed(lambda: cops.plane_stats(x)), 4)
    st = cops.plane_stats(x)
    out["fold_128_ms"] = round(timed(lambda: cops.fold(st, 128, L * L, eps=1e-6)), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
