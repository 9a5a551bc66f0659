"""Contact-head benchmark (outside the metric): the batched head body with its launches issued from C
(``body_batch(native=True)``: di_head_body_batch + di_head_logits_batch, what ``head_body="native"``
runs) against the same launches issued from Python (``body_batch``, what ``head_body="python"`` runs),
in one process on the same inputs. bf16, HIP convolutions, seeded weights; the inputs are B prologue
outputs [1, 128, side, side] (ELU of a normal sample).

Cases: side 64, 145, 256 at B = 1, 4, 16, and 1000 at B = 2 (kernel-bound: expected level). The method is
tools/bench_head_batch.py's: HIP events on one stream; every case is warmed up, then the two sides are
timed in alternating windows of `--reps` forwards and the median window is reported with the fastest
and slowest (ms per forward over all B complexes). Both sides build their HeadBatch and copy the inputs
in inside the timed region, as LitGINI._head_batched does per chunk. ``launches`` counts the device
kernels of one forward on each side (torch.profiler; the input copies are B of them on either side).
``max_abs_diff`` compares the two sides' logits (they share every bit up to phase2_conv's input).
Needs a GPU: there is no CPU path.

``--forwards B:side:N`` runs 2 + N native forwards of one case and nothing else, and prints the host's
enqueue time and the wall time per forward: the run to put under ``rocprofv3 --kernel-trace --stats``
(profiles/head_native_kernel_stats_<side>.csv are its kernel statistics for 1:64:20, 1:145:10, 1:1000:3).

usage: python tools/bench_head_native.py [--reps 2] [--windows 5] [--out profiles/head_native_bench.json]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_head_native.py --forwards 1:64:20
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_head_batch import head, launches, window  # noqa: E402

CASES = tuple((b, side) for side in (64, 145, 256) for b in (1, 4, 16)) + ((2, 1000),)


def measure(native, python, reps, windows):
    for fn in (native, python):  # warm-up: code objects, allocator, the plan
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t_n, t_p = [], []
    for _ in range(windows):
        t_n.append(window(native, reps))
        t_p.append(window(python, reps))
    m_n, m_p = statistics.median(t_n), statistics.median(t_p)
    return {"native_ms": m_n, "native_ms_min_max": [min(t_n), max(t_n)], "python_ms": m_p,
            "python_ms_min_max": [min(t_p), max(t_p)], "python_over_native": m_p / m_n}


def forwards(m, count, side, n):
    """2 + n native forwards of one case (for a kernel trace): host enqueue and wall ms per forward."""
    g = torch.Generator(device="cuda").manual_seed(0)
    xs = [F.elu(torch.randn(1, 128, side, side, generator=g, device="cuda")).to(torch.bfloat16) for _ in range(count)]
    with torch.no_grad():
        for _ in range(2):
            m.body_batch(xs, native=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            m.body_batch(xs, native=True)
        host = time.perf_counter() - t
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
    print(json.dumps({"complexes": count, "shape": [side, side], "forwards": n, "host_enqueue_ms": host / n * 1e3,
                      "wall_ms": wall / n * 1e3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--cases", default="", help="B:side,... (default: the documented set)")
    ap.add_argument("--forwards", default="", help="B:side:N: only 2 + N native forwards of this case (for a trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_native_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_native needs a ROCm GPU")
    if a.forwards:
        return forwards(head(), *(int(v) for v in a.forwards.split(":")))
    cases = tuple(tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")) if a.cases else CASES
    m = head()
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    with torch.no_grad():
        for count, side in cases:
            xs = [F.elu(torch.randn(1, 128, side, side, generator=g, device="cuda")).to(torch.bfloat16)
                  for _ in range(count)]

            def native():
                return m.body_batch(xs, native=True)

            def python():
                return m.body_batch(xs)

            row = {"complexes": count, "shape": [side, side]}
            row.update(measure(native, python, a.reps, a.windows))
            row["launches"] = {"native": launches(native), "python": launches(python)}
            row["ms_per_complex"] = {"native": row["native_ms"] / count, "python": row["python_ms"] / count}
            row["max_abs_diff"] = max(float((n.float() - p.float()).abs().max()) for n, p in zip(native(), python()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del xs
            torch.cuda.empty_cache()
    out = {"workload": "contact-head body (56 + 6 ResNet blocks + phase2_conv), bf16, HIP convolutions, over B "
                       "complexes: launches issued by di_head_body_batch + di_head_logits_batch (native) vs by "
                       "ResNet._forward_hipconv_batch + torch's ELU and phase2_conv (python)",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "timing": "HIP events on the current stream, alternating windows, median window, ms per forward over all "
                     "B complexes; HeadBatch construction and input copies inside the window",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
