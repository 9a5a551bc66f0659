"""Example-list benchmark (outside the metric): ranking.ExamplesOp.labels (one memset and one launch for
all complexes, csrc/contact_examples.hip) against ranking.labels_from_examples_batch_torch (a loop of
about a dozen torch kernels per complex) on the same device tensors, and what the test loop gains.

Cases: 32 x 145^2, 32 x 300^2, 8 x 1000^2 and one 1000^2 complex, each with the rows in row-major order
and shuffled; int64 lists, labels at 1 %. HIP events on one stream; every case is warmed up, then the
two sides are timed in alternating windows of `--reps` calls and the median window is reported with the
fastest and slowest (ms per call over the whole set of complexes). Rows per case:
  labels          the label maps, validated: both sides end with their one host read of the flags
  test_loop       labels + ContactRankOp.batch + ContactAucOp.batch + the host reads of every
                  complex's figures (tools/eval_bench.py's "both_with_reads", the labels' time
                  included on both sides)
  gather          (row-major order only) ExamplesOp.gather of a 10 % sample of every complex, one pool
                  per complex, validated and read, against torch indexing of the same lists
                  (flatten, index, transpose as the reference's validation_step does; no validation,
                  one synchronisation)
Needs a GPU: there is no CPU path. --lib times a variant build of the library
(deepinteract_amd.build.build_variant) in place of the in-tree one.

usage: python tools/examples_bench.py [--reps 10] [--windows 7] [--out profiles/examples_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((32, 145), (32, 300), (8, 1000), (1, 1000))
SHARE = 0.01
SAMPLE = 0.1


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def measure(op_side, torch_side, reps, windows):
    for fn in (op_side, torch_side):  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t_o, t_t = [], []
    for _ in range(windows):
        t_o.append(window(op_side, reps))
        t_t.append(window(torch_side, reps))
    m_o, m_t = statistics.median(t_o), statistics.median(t_t)
    return {"op_ms": m_o, "op_ms_min_max": [min(t_o), max(t_o)], "torch_ms": m_t,
            "torch_ms_min_max": [min(t_t), max(t_t)], "torch_over_op": m_t / m_o}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "examples_bench.json"))
    ap.add_argument("--lib", default=None, help="a variant library to time instead of the in-tree one")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("examples_bench needs a ROCm GPU")
    if a.lib:
        from deepinteract_amd import _lib
        _lib.load_variant(a.lib)
    from deepinteract_amd.ranking import ContactAucOp, ContactRankOp, ExamplesOp, labels_from_examples_batch_torch
    ex_op, rank, auc = ExamplesOp("cuda"), ContactRankOp("cuda"), ContactAucOp("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for count, side in CASES:
        n = side * side
        shapes = [(side, side)] * count
        logits = []
        for _ in range(count):
            lg = 6.0 * torch.randn(1, 2, side, side, generator=g, device="cuda")
            lg[:, 1] -= 7.0
            logits.append(lg)
        i, j = torch.meshgrid(torch.arange(side, device="cuda"), torch.arange(side, device="cuda"), indexing="ij")
        for order in ("row_major", "shuffled"):
            lists = []
            for _ in range(count):
                lab = (torch.rand(n, generator=g, device="cuda") < SHARE).long()
                ex = torch.stack((i.flatten(), j.flatten(), lab), dim=1)
                if order == "shuffled":
                    ex = ex[torch.randperm(n, generator=g, device="cuda")]
                lists.append(ex.contiguous())
            same = all(torch.equal(x, y) for x, y in zip(ex_op.labels(lists, shapes),
                                                         labels_from_examples_batch_torch(lists, shapes)))

            def loop(labels_fn):
                labels = labels_fn(lists, shapes)
                rs = rank.batch(logits, labels_list=labels)
                aus = auc.batch([r.probs for r in rs], labels)
                return [r.metrics() for r in rs], [x.metrics() for x in aus]

            row = {"complexes": count, "shape": [side, side], "order": order, "positives_share": SHARE,
                   "op_equals_torch": bool(same),
                   "labels": measure(lambda: ex_op.labels(lists, shapes),
                                     lambda: labels_from_examples_batch_torch(lists, shapes), a.reps, a.windows),
                   "test_loop": measure(lambda: loop(ex_op.labels), lambda: loop(labels_from_examples_batch_torch),
                                        a.reps, a.windows)}
            if order == "row_major":
                rows_kept = max(1, int(n * SAMPLE))
                sampled = [ex[torch.randint(0, n, (rows_kept,), generator=g, device="cuda")].contiguous() for ex in lists]

                def torch_gather():
                    out = []
                    for lg, ex in zip(logits, sampled):
                        idx = ex[:, 1] + lg.shape[3] * ex[:, 0]
                        out.append((torch.flatten(lg[0], start_dim=1)[:, idx].transpose(1, 0), ex[:, 2]))
                    torch.cuda.synchronize()
                    return out

                got = ex_op.gather(logits, sampled)
                row["gather_equals_torch"] = all(torch.equal(pl.view(2, -1).t(), want) for (pl, _), (want, _)
                                                 in zip(got, torch_gather()))
                row["gather_rows_per_complex"] = rows_kept
                row["gather"] = measure(lambda: ex_op.gather(logits, sampled), torch_gather, a.reps, a.windows)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"workload": "example lists of a set of complexes as label maps / pooled samples: ExamplesOp vs torch",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "library": a.lib or "in-tree",
           "timing": "HIP events on the current stream, median window, ms per call over all complexes",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
