"""Test-loop benchmark (outside the metric): the batched ranking / AUC calls (ContactRankOp.batch,
ContactAucOp.batch: one launch sequence for all complexes) against a loop of the single-complex calls
over the same inputs, which is what LitGINI.test_step does per complex.

Cases: 32 x 145^2, 32 x 300^2, 8 x 1000^2 and a batch of one 1000^2; logits 6 randn with class 1 shifted
by -7 (saturated: exact ties), labels at 1 %. HIP events on one stream; every case is warmed up, then
the two sides are timed in alternating windows of `--reps` calls and the median window is reported
with the fastest and slowest (ms per call over the whole set of complexes). Rows per case:
  rank            the ranking calls alone, both sides asynchronous inside a window
  auc             the AUC calls alone (on the maps the ranking stored), asynchronous
  both_with_reads ranking + AUC + the host reads of every complex's figures (the batch reads two
                  metrics tables; the loop reads two records per complex)
Needs a GPU: there is no CPU path.

usage: python tools/eval_bench.py [--reps 10] [--windows 7] [--out profiles/eval_bench.json]
       python tools/eval_bench.py --probe-one     # where a batch of one differs from the single call
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

CASES = ((32, 145), (32, 300), (8, 1000), (1, 1000))
SHARE = 0.01


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def measure(batched, loop, reps, windows):
    for fn in (batched, loop):  # warm-up: code objects, allocator, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t_b, t_l = [], []
    for _ in range(windows):
        t_b.append(window(batched, reps))
        t_l.append(window(loop, reps))
    m_b, m_l = statistics.median(t_b), statistics.median(t_l)
    return {"batch_ms": m_b, "batch_ms_min_max": [min(t_b), max(t_b)], "loop_ms": m_l,
            "loop_ms_min_max": [min(t_l), max(t_l)], "loop_over_batch": m_l / m_b}


def probe_one(reps=50, windows=7):
    """Where a batch of ONE differs from the single call at 1000 x 1000: the descriptor table's copy
    alone, the C entry points alone (tables prepared once, outputs reused), and the Python ops; in
    alternating windows, [median, fastest, slowest] ms per call."""
    import ctypes

    from deepinteract_amd import _lib
    from deepinteract_amd.engine import _ptr, _stream
    from deepinteract_amd.ranking import _table_to_device
    rank, auc = ContactRankOp("cuda"), ContactAucOp("cuda")
    lib = rank.lib
    g = torch.Generator(device="cuda").manual_seed(0)
    side, n, k = 1000, 10 ** 6, 1000
    lg = 6.0 * torch.randn(1, 2, side, side, generator=g, device="cuda")
    lg[:, 1] -= 7.0
    lab = (torch.rand(n, generator=g, device="cuda") < SHARE).to(torch.uint8)
    r = rank(lg, labels=lab)
    probs, ids, scores, hits = r.probs, r.ids, r.scores, r.hits
    met = torch.empty(6, dtype=torch.int64, device="cuda")
    amet = torch.empty(8, dtype=torch.int64, device="cuda")
    max_pos = ContactAucOp.default_max_pos(n)
    items = (_lib.DiRankItem * 1)()
    it = items[0]
    it.logits, it.labels, it.probs, it.top_ids, it.top_scores, it.top_hits, it.metrics = (
        t.data_ptr() for t in (lg, lab, probs, ids, scores, hits, met))
    it.l1, it.l2, it.k = side, side, k
    work = torch.empty(lib.di_contact_rank_batch_work_bytes(items, 1) // 8 + 1, dtype=torch.int64, device="cuda")
    items_dev = _table_to_device(items, rank.device)
    aitems = (_lib.DiAucItem * 1)()
    a = aitems[0]
    a.probs, a.labels, a.out, a.n, a.max_pos = probs.data_ptr(), lab.data_ptr(), amet.data_ptr(), n, max_pos
    awork = torch.empty(lib.di_contact_auc_batch_work_bytes(aitems, 1) // 8 + 1, dtype=torch.int64, device="cuda")
    aitems_dev = _table_to_device(aitems, rank.device)
    thr = ctypes.c_float(0.5)
    fns = {
        "table_copy_alone": lambda: _table_to_device(items, rank.device),
        "c_rank_single": lambda: lib.di_contact_rank(_lib.DI_F32, _ptr(lg), side, side, k, _ptr(lab), thr,
                                                     _ptr(probs), _ptr(ids), _ptr(scores), _ptr(hits), _ptr(met),
                                                     _ptr(work), _stream()),
        "c_rank_batch_of_one": lambda: lib.di_contact_rank_batch(_lib.DI_F32, items, _ptr(items_dev), 1, thr,
                                                                 _ptr(work), _stream()),
        "c_auc_single": lambda: lib.di_contact_auc(_ptr(probs), _ptr(lab), n, max_pos, _ptr(amet), _ptr(awork),
                                                   _stream()),
        "c_auc_batch_of_one": lambda: lib.di_contact_auc_batch(aitems, _ptr(aitems_dev), 1, _ptr(awork), _stream()),
        "py_rank_single": lambda: rank(lg, labels=lab),
        "py_rank_batch_of_one": lambda: rank.batch([lg], labels_list=[lab]),
        "py_auc_single": lambda: auc(probs, lab),
        "py_auc_batch_of_one": lambda: auc.batch([probs], [lab]),
    }
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            t[name].append(window(fn, reps))
    return {name: [statistics.median(v), min(v), max(v)] for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--probe-one", action="store_true",
                    help="only time a batch of one 1000 x 1000 complex against the single call, layer by layer")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a ROCm GPU")
    if a.probe_one:
        print(json.dumps(probe_one(), indent=1))
        return
    rank, auc = ContactRankOp("cuda"), ContactAucOp("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for count, side in CASES:
        logits, labels = [], []
        for _ in range(count):
            lg = 6.0 * torch.randn(1, 2, side, side, generator=g, device="cuda")
            lg[:, 1] -= 7.0
            logits.append(lg)
            labels.append((torch.rand(side * side, generator=g, device="cuda") < SHARE).to(torch.uint8))
        probs = [r.probs for r in rank.batch(logits, labels_list=labels)]
        same = all(x.metrics() == y.metrics() for x, y in zip(rank.batch(logits, labels_list=labels),
                                                              [rank(lg, labels=lab) for lg, lab in zip(logits, labels)]))
        same = same and all(x.metrics() == y.metrics() for x, y in
                            zip(auc.batch(probs, labels), [auc(p, lab) for p, lab in zip(probs, labels)]))

        def rank_batch():
            return rank.batch(logits, labels_list=labels)

        def rank_loop():
            return [rank(lg, labels=lab) for lg, lab in zip(logits, labels)]

        def auc_batch():
            return auc.batch(probs, labels)

        def auc_loop():
            return [auc(p, lab) for p, lab in zip(probs, labels)]

        def both_batch():
            rs = rank.batch(logits, labels_list=labels)
            aus = auc.batch([r.probs for r in rs], labels)
            return [r.metrics() for r in rs], [x.metrics() for x in aus]

        def both_loop():
            out = []
            for lg, lab in zip(logits, labels):
                r = rank(lg, labels=lab)
                x = auc(r.probs, lab)
                out.append((r.metrics(), x.metrics()))
            return out

        rows.append({"complexes": count, "shape": [side, side], "positives_share": SHARE,
                     "batch_equals_loop": bool(same),
                     "rank": measure(rank_batch, rank_loop, a.reps, a.windows),
                     "auc": measure(auc_batch, auc_loop, a.reps, a.windows),
                     "both_with_reads": measure(both_batch, both_loop, a.reps, a.windows)})
    out = {"workload": "ranking + exact AUROC / AUPRC of a set of complexes: one batched call vs a loop of single calls",
           "device": torch.cuda.get_device_name(0), "reps_per_window": a.reps, "windows": a.windows,
           "timing": "HIP events on the current stream, median window, ms per call over all complexes",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
