#!/usr/bin/env python3
"""What ``predict_sharded(gather="topk")`` saves against the map modes, measured in ONE process group.

For N synthetic complexes the sharded driver runs with gather = "once", "chunked" and "topk" (records
of ids and scores) and "topk" with labels (records that also carry top_hits and test_step's
metrics; the forward then reads example lists and runs the AUC op too), interleaved in the same
process, fastest of --reps runs each. Per mode:

* bytes sent per rank and receive-buffer bytes per rank: derived from the plan and the layout
  (``di_rank_record_bytes``), not measured;
* wall time of the call (max over ranks);
* the collective's exposed time, as ``bench.py --dist``'s allgather_record measures it: the call's
  time minus the time of the same compute without any collective (gather="none" for the map modes;
  for topk the same forward writing the same send buffer, the all-gather left out).

World size: whatever the launcher gives (``torchrun --nproc_per_node=G tools/bench_sharded_topk.py``);
started plainly it is a group of one RCCL rank, and then the collective moves nothing between GPUs: the
JSON says that the wire time could not be measured. The byte figures hold for any world size.

    python tools/bench_sharded_topk.py --complexes 8 --n-res 512 --out profiles/sharded_topk_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def max_over_ranks(x, dev):
    t = torch.tensor([x], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t)


def full_examples(l1, l2, share, seed, dev):
    g = torch.Generator().manual_seed(seed)
    i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
    lab = (torch.rand(l1 * l2, generator=g) < share).long()
    return torch.stack((i.flatten(), j.flatten(), lab), dim=1).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--complexes", type=int, default=8, help="complexes per rank")
    ap.add_argument("--n-res", type=int, default=512, help="residues per chain")
    ap.add_argument("--micro-batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    rank, ws = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", rank=rank, world_size=ws, device_id=dev)

    from deepinteract_amd import _lib, synth
    from deepinteract_amd.distributed import (RecordPlan, gather_rounds, gpu_forward, local_order, predict_sharded,
                                              ranked_forward, shard)
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.ranking import RecordSlot
    from deepinteract_amd.weights import seeded_state_dict

    model = LitGINI(dtype="bf16", head_dtype=torch.bfloat16).to(dev).eval()
    model.load_reference_state_dict(seeded_state_dict(0))
    n, mb = args.n_res, args.micro_batch
    cx = [synth.synthetic_complex(60_000 + i, n, n) for i in range(args.complexes * ws)]
    sizes = [(n, n)] * len(cx)
    plan = shard(sizes, ws)
    examples = [full_examples(n, n, 0.01, i, dev) for i in range(len(cx))]
    forwards = {"maps": gpu_forward(model, 20), "topk": ranked_forward(model, 20),
                "topk_labels": ranked_forward(model, 20, examples=examples)}

    def topk_compute_only(with_labels):
        """predict_sharded(gather="topk") without its collective: the same forward, the same send buffer."""
        rp = RecordPlan(sizes, plan, None, with_labels)
        send = torch.zeros(rp.width // 4, dtype=torch.int32, device=dev)
        mine = local_order(sizes, plan[rank])
        fwd = forwards["topk_labels" if with_labels else "topk"]
        for s in range(0, len(mine), mb):
            ids = mine[s:s + mb]
            fwd([cx[i] for i in ids], ids, out=[RecordSlot(send, rp.place[i][1], n, n, rp.ks[i], with_labels)
                                                 for i in ids])

    runs = {
        "none": lambda: predict_sharded(cx, forwards["maps"], micro_batch=mb, device=dev, gather="none"),
        "once": lambda: predict_sharded(cx, forwards["maps"], micro_batch=mb, device=dev, gather="once"),
        "chunked": lambda: predict_sharded(cx, forwards["maps"], micro_batch=mb, device=dev, gather="chunked"),
        "topk": lambda: predict_sharded(cx, forwards["topk"], micro_batch=mb, device=dev, gather="topk"),
        "topk_none": lambda: topk_compute_only(False),
        "topk_labels": lambda: predict_sharded(cx, forwards["topk_labels"], micro_batch=mb, device=dev, gather="topk",
                                               with_labels=True),
        "topk_labels_none": lambda: topk_compute_only(True),
    }

    def timed(name):
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runs[name]()
        torch.cuda.synchronize()
        return max_over_ranks(time.perf_counter() - t0, dev)

    for name in runs:            # one untimed run each: buffers, workspaces, RCCL set-up
        timed(name)
    best = {}
    for _ in range(args.reps):   # interleaved, the fastest run of each kept
        for name in runs:
            best[name] = min(best.get(name, float("inf")), timed(name))

    maps_el = [sum(a * b for a, b in (sizes[i] for i in p)) for p in plan]
    rounds = gather_rounds(sizes, plan, mb)
    sent = {"once": 4 * max(max(maps_el), 1), "chunked": 4 * sum(w for _, w in rounds)}
    for name, with_labels in (("topk", False), ("topk_labels", True)):
        sent[name] = RecordPlan(sizes, plan, None, with_labels).send_bytes
    base = {"once": "none", "chunked": "none", "topk": "topk_none", "topk_labels": "topk_labels_none"}
    modes = {}
    for name in ("once", "chunked", "topk", "topk_labels"):
        modes[name] = {"sent_bytes_per_rank": sent[name], "recv_buffer_bytes_per_rank": ws * sent[name],
                       "wall_s": round(best[name], 5), "compute_only_s": round(best[base[name]], 5),
                       "exposed_collective_s": round(max(best[name] - best[base[name]], 0.0), 5)}
    rec_1000 = _lib.rank_record_layout(1000, 1000, 1000, True)[0]
    out = {
        "tool": "tools/bench_sharded_topk.py", "device": torch.cuda.get_device_name(dev), "world_size": ws,
        "complexes": len(cx), "shape": [n, n], "micro_batch": mb, "reps": args.reps,
        "model": "LitGINI bf16 GeoT + bf16 head, seeded weights; synthetic complexes, 1 % positives",
        "record_bytes": {"topk": _lib.rank_record_layout(n, n, n, False)[0],
                         "topk_labels": _lib.rank_record_layout(n, n, n, True)[0], "map_fp32": 4 * n * n},
        "modes": modes,
        "layout_1000x1000_k1000_labels": {"record_bytes": rec_1000, "map_bytes": 4_000_000,
                                          "recv_bytes_per_rank_8192_complexes": {"topk": 8192 * rec_1000,
                                                                                 "maps": 8192 * 4_000_000}},
        "wire_time": ("measured: exposed_collective_s is the all-gather's cost across the ranks" if ws > 1 else
                      "NOT measured: a group of one rank moves nothing between GPUs; exposed_collective_s is the "
                      "local copy and launch cost only. Byte and buffer figures follow from the layout and hold."),
    }
    if rank == 0:
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
