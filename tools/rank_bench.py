"""Contact-ranking benchmark (outside the metric): ranking.ContactRankOp against the line a user writes
without it,

    torch.softmax(lg.squeeze(0), 0)[1].flatten().topk(K, sorted=True)

on the same device and the same logits (6 randn, class 1 shifted by -7: a saturated map with exact
ties), at 1000 x 1000 (K = 1000) and 4096 x 4096 (K = 4096), fp32 and bf16. HIP events on one stream;
every shape is warmed up, then the two sides are timed in alternating windows of `--reps` calls and
the median window is reported with the fastest and slowest (ms per call). Also the op's algorithmic
bytes per element (csrc/contact_rank.hip) and the share of the HBM peak they amount to at the measured
time. Needs a GPU: there is no CPU path.

usage: python tools/rank_bench.py [--reps 50] [--windows 7] [--out profiles/rank_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepinteract_amd.ranking import ContactRankOp  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, the MI355X's specified HBM3E bandwidth
SHAPES = ((1000, 1000, 1000), (4096, 4096, 4096))


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def algorithmic_bytes_per_element(dtype, labels=False):
    """k_rank_probs reads both class planes and writes the fp32 map (+ 1 label byte); the two later
    histogram passes and the count pass read the map; the compaction and the one-block stages touch
    O(K) elements."""
    return 2 * (2 if dtype == torch.bfloat16 else 4) + 4 + (1 if labels else 0) + 3 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs a ROCm GPU")
    op = ContactRankOp("cuda")
    rows = []
    for l1, l2, k in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        base = 6.0 * torch.randn(1, 2, l1, l2, generator=g, device="cuda")
        base[:, 1] -= 7.0
        for dtype in (torch.float32, torch.bfloat16):
            lg = base.to(dtype).contiguous()
            probs = torch.empty(l1, l2, dtype=torch.float32, device="cuda")

            def run_op():
                return op(lg, k=k, probs_out=probs)

            def run_torch():
                return torch.softmax(lg.squeeze(0), 0)[1].flatten().topk(k, sorted=True)

            for fn in (run_op, run_torch):  # warm-up: code objects, allocator, workspace
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            t_op, t_torch = [], []
            for _ in range(a.windows):
                t_op.append(window(run_op, a.reps))
                t_torch.append(window(run_torch, a.reps))
            m_op, m_torch = statistics.median(t_op), statistics.median(t_torch)
            bpe = algorithmic_bytes_per_element(dtype)
            n = l1 * l2
            rows.append({"shape": [l1, l2], "k": k, "dtype": str(dtype).replace("torch.", ""),
                         "op_ms": m_op, "op_ms_min_max": [min(t_op), max(t_op)],
                         "torch_ms": m_torch, "torch_ms_min_max": [min(t_torch), max(t_torch)],
                         "torch_over_op": m_torch / m_op,
                         "op_bytes_per_element": bpe,
                         "op_algorithmic_GBps": bpe * n / (m_op * 1e-3) / 1e9,
                         "op_share_of_hbm_peak": bpe * n / (m_op * 1e-3) / HBM_PEAK})
    out = {"workload": "contact ranking of one complex: ContactRankOp vs softmax + topk in torch",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "timing": "HIP events on the current stream, median window, ms per call", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
