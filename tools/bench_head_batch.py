"""Contact-head benchmark (outside the metric): the batched head body
(ResNet2DInputWithOptAttention.body_batch: every head kernel launched once for B complexes) against a
loop of the single-complex ``body`` over the same inputs -- the path ``head_convs="hip"`` takes without
``head_batch``. bf16, HIP convolutions, seeded weights; the inputs are B prologue outputs
[1, 128, side, side] (ELU of a normal sample).

Cases: side 64, 145, 256 at B = 1, 4, 16, 64, and 1000 at B = 2 (where nothing is expected to change).
HIP events on one stream; every case is warmed up, then the two sides are timed in alternating windows
of `--reps` forwards and the median window is reported with the fastest and slowest (ms per forward
over all B complexes). The batch side builds its HeadBatch and copies the inputs in inside the timed
region, as LitGINI._forward_batch does per chunk. ``launches`` counts the device kernels of one forward
on each side (torch.profiler). Needs a GPU: there is no CPU path.

--f32: the fp32 parity head instead (head_convs="hip_f32": fp32 storage and weights, di_head_conv_f32 and
the *_f32_batch passes; what head_batch_f32 runs per chunk) against a loop of single hip_f32 ``body`` calls
in the same process, over 16 x 64^2, 16 x 145^2, 16 x 256^2 and 2 x 1000^2, into
profiles/head_batch_f32_bench.json.

usage: python tools/bench_head_batch.py [--f32] [--reps 2] [--windows 5] [--out profiles/head_batch_bench.json]
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

from deepinteract_amd.head import HeadConvOps, HeadNormOps, ResNet2DInputWithOptAttention  # noqa: E402
from deepinteract_amd.weights import seeded_state_dict  # noqa: E402

CASES = tuple((b, side) for side in (64, 145, 256) for b in (1, 4, 16, 64)) + ((2, 1000),)
CASES_F32 = ((16, 64), (16, 145), (16, 256), (2, 1000))


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def measure(batched, loop, reps, windows):
    for fn in (batched, loop):  # warm-up: code objects, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t_b, t_l = [], []
    for _ in range(windows):
        t_b.append(window(batched, reps))
        t_l.append(window(loop, reps))
    m_b, m_l = statistics.median(t_b), statistics.median(t_l)
    return {"batch_ms": m_b, "batch_ms_min_max": [min(t_b), max(t_b)], "loop_ms": m_l,
            "loop_ms_min_max": [min(t_l), max(t_l)], "loop_over_batch": m_l / m_b}


def launches(fn):
    """Device kernels of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())


def head(dtype=torch.bfloat16):
    sd = seeded_state_dict(0)
    hsd = {k[len("interact_module."):]: v for k, v in sd.items() if k.startswith("interact_module.")}
    m = ResNet2DInputWithOptAttention().cuda().eval()
    m.load_state_dict(hsd)
    m = m.to(dtype=dtype)
    return m.use_hip_norm_ops(HeadNormOps("cuda")).use_hip_convs(HeadConvOps("cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--cases", default="", help="B:side,... (default: the documented set)")
    ap.add_argument("--f32", action="store_true", help="the fp32 parity head (hip_f32) and its documented cases")
    ap.add_argument("--out", default="", help="default: profiles/head_batch_bench.json (--f32: "
                                              "profiles/head_batch_f32_bench.json)")
    a = ap.parse_args()
    dtype = torch.float32 if a.f32 else torch.bfloat16
    out_path = a.out or os.path.join(ROOT, "profiles", "head_batch_f32_bench.json" if a.f32 else "head_batch_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_batch needs a ROCm GPU")
    cases = tuple(tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")) if a.cases else \
        (CASES_F32 if a.f32 else CASES)
    m = head(dtype)
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    with torch.no_grad():
        for count, side in cases:
            xs = [F.elu(torch.randn(1, 128, side, side, generator=g, device="cuda")).to(dtype)
                  for _ in range(count)]

            def batched():
                return m.body_batch(xs)

            def loop():
                return [m.body(x) for x in xs]

            row = {"complexes": count, "shape": [side, side]}
            row.update(measure(batched, loop, a.reps, a.windows))
            row["launches"] = {"batch": launches(batched), "loop": launches(loop)}
            row["ms_per_complex"] = {"batch": row["batch_ms"] / count, "loop": row["loop_ms"] / count}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xs
            torch.cuda.empty_cache()
    kind = "fp32 (hip_f32)" if a.f32 else "bf16"
    out = {"workload": f"contact-head body (58 + 4 ResNet blocks + phase2_conv), {kind}, HIP convolutions: body_batch "
                       "over B complexes vs a loop of B single-complex body calls",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "timing": "HIP events on the current stream, median window, ms per forward over all B complexes",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
