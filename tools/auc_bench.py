"""Contact-AUC benchmark (outside the metric): ranking.ContactAucOp against an exact formulation of
the same two figures a user writes in torch without it, on the same device and the same map:

    vals, idx = torch.sort(p, descending=True); y = labels[idx]
    tp, fp = cumsum(y), cumsum(1 - y); last = last element of every run of equal vals
    auroc = trapezoid of (fp[last] / N, tp[last] / P) from (0, 0); auprc = sum diff(tp[last]) / P * tp / (tp + fp)

(a full sort of the map plus cumsums, fp64 arithmetic), at 1000 x 1000 and 4096 x 4096 with 0.5 % and
2 % positives. The map is the one ContactRankOp stores for 6 randn logits with class 1 shifted by -7
(saturated: exact ties). HIP events on one stream; every case is warmed up, then the two sides are
timed in alternating windows of `--reps` calls and the median window is reported with the fastest and
slowest (ms per call). Both sides stay asynchronous inside a window (no host read of the figures).
Also the op's algorithmic bytes per element (csrc/contact_auc.hip) and the share of the HBM peak they
amount to at the measured time. Needs a GPU: there is no CPU path.

usage: python tools/auc_bench.py [--reps 20] [--windows 7] [--out profiles/auc_bench.json]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
           python tools/auc_bench.py --calls-only 4096 0.02     # 20 op calls at one case: per-kernel times
           (profiles/auc_kernel_stats_4096.csv, profiles/auc_kernel_stats_1000.csv)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepinteract_amd.ranking import ContactAucOp, ContactRankOp  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, the MI355X's specified HBM3E bandwidth
SHAPES = ((1000, 1000), (4096, 4096))
SHARES = (0.005, 0.02)
OP_BYTES_PER_ELEMENT = 2 * (4 + 1)  # two passes over the fp32 map and its uint8 labels


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_exact(p, labels):
    """(auroc, auprc) as 0-d fp64 device tensors: full sort, cumsums, tie groups."""
    vals, idx = torch.sort(p, descending=True)
    y = labels[idx].to(torch.int64)
    tp, fp = torch.cumsum(y, 0), torch.cumsum(1 - y, 0)
    last = torch.ones_like(vals, dtype=torch.bool)
    last[:-1] = vals[1:] != vals[:-1]
    tp, fp = tp[last].double(), fp[last].double()
    P, N = tp[-1], fp[-1]
    zero = torch.zeros(1, dtype=torch.float64, device=p.device)
    tp0, fp0 = torch.cat((zero, tp)), torch.cat((zero, fp))
    auroc = ((fp0[1:] - fp0[:-1]) * (tp0[1:] + tp0[:-1])).sum() / (2 * P * N)
    auprc = ((tp0[1:] - tp0[:-1]) * tp / (tp + fp)).sum() / P
    return auroc, auprc


def case_map(rank, l1, l2):
    g = torch.Generator(device="cuda").manual_seed(0)
    lg = 6.0 * torch.randn(1, 2, l1, l2, generator=g, device="cuda")
    lg[:, 1] -= 7.0
    return rank(lg, k=10).probs, g


def case_labels(n, share, g):
    return (torch.rand(n, generator=g, device="cuda") < share).to(torch.uint8)


def calls_only(op, rank, side, share, calls=20):
    probs, g = case_map(rank, side, side)
    labels = case_labels(side * side, share, g)
    res = op(probs, labels)
    print(json.dumps({"shape": [side, side], "positives_share": share, "max_pos": res.max_pos, **res.metrics()}))
    for _ in range(calls):
        op._run(probs, labels, res.max_pos)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc_bench.json"))
    ap.add_argument("--calls-only", nargs=2, metavar=("SIDE", "SHARE"),
                    help="run 20 op calls on a SIDE x SIDE map with SHARE positives and exit (for a profiler)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("auc_bench needs a ROCm GPU")
    op, rank = ContactAucOp("cuda"), ContactRankOp("cuda")
    if a.calls_only:
        return calls_only(op, rank, int(a.calls_only[0]), float(a.calls_only[1]))
    rows = []
    for l1, l2 in SHAPES:
        n = l1 * l2
        probs, g = case_map(rank, l1, l2)
        flat = probs.view(-1)
        for share in SHARES:
            labels = case_labels(n, share, g)
            res = op(probs, labels)
            m = dict(res.metrics())                      # also settles max_pos (no overflow inside the windows)
            max_pos = res.max_pos
            t_roc, t_ap = (float(x) for x in torch_exact(flat, labels))

            def run_op():
                return op._run(probs, labels, max_pos)

            def run_torch():
                return torch_exact(flat, labels)

            for fn in (run_op, run_torch):  # warm-up: code objects, allocator, workspace
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t_op, t_torch = [], []
            for _ in range(a.windows):
                t_op.append(window(run_op, a.reps))
                t_torch.append(window(run_torch, a.reps))
            m_op, m_torch = statistics.median(t_op), statistics.median(t_torch)
            rows.append({"shape": [l1, l2], "positives_share": share, "num_pos": m["num_pos"],
                         "pos_distinct": m["pos_distinct"], "max_pos": max_pos,
                         "auroc": m["auroc"], "auprc": m["auprc"],
                         "torch_auroc_rel_diff": abs(t_roc - m["auroc"]) / m["auroc"],
                         "torch_auprc_rel_diff": abs(t_ap - m["auprc"]) / m["auprc"],
                         "op_ms": m_op, "op_ms_min_max": [min(t_op), max(t_op)],
                         "torch_ms": m_torch, "torch_ms_min_max": [min(t_torch), max(t_torch)],
                         "torch_over_op": m_torch / m_op,
                         "op_bytes_per_element": OP_BYTES_PER_ELEMENT,
                         "op_algorithmic_GBps": OP_BYTES_PER_ELEMENT * n / (m_op * 1e-3) / 1e9,
                         "op_share_of_hbm_peak": OP_BYTES_PER_ELEMENT * n / (m_op * 1e-3) / HBM_PEAK})
    out = {"workload": "exact AUROC / AUPRC of one complex: ContactAucOp vs torch.sort + cumsums",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "timing": "HIP events on the current stream, median window, ms per call", "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
