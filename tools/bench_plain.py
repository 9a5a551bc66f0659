"""GeoT benchmark of disable_geometric_mode (outside the metric): the plain Graph Transformer engine
(csrc/geot_plain.hip) beside the geometric engine on the C3 shape -- 8 device-built complexes of 2 x 1000
residues, k = 20 (16000 nodes, 320000 edges) -- through GeoTEngine.forward(events=...), seeded weights.

Per dtype (bf16, fp32) one plain and one geometric engine run in ONE process on the same batch: after
``--warmup`` forwards of each, ``--rounds`` rounds alternate plain and geometric forwards, every launch
between HIP events on the launch stream. Reported per engine and kernel name: the median over the
rounds of that round's summed time (ms), with the fastest and slowest round. ``edge_ms`` is edge_layer +
edge_layer_final, the figure the two modes are compared on: the plain layers run 6 + 2 weight stages
against the geometric layers' 17 - 22 and gather no neighbour rows, so ``plain_edge_le_geometric`` is
expected to hold; the script exits 1 if it does not. Needs a GPU: there is no CPU path.

usage: python tools/bench_plain.py [--rounds 20] [--warmup 5] [--complexes 8] [--residues 1000]
                                   [--out profiles/geot_plain_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deepinteract_amd import synth  # noqa: E402
from deepinteract_amd.builder import build_graph_batch  # noqa: E402
from deepinteract_amd.config import GeoTConfig  # noqa: E402
from deepinteract_amd.engine import GeoTEngine  # noqa: E402
from deepinteract_amd.weights import seeded_state_dict  # noqa: E402


def one_forward(eng, gb):
    """kernel name -> summed ms of one forward's launches of that name"""
    events = {}
    eng.forward(gb, clone=False, events=events)
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--complexes", type=int, default=8)
    ap.add_argument("--residues", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geot_plain_bench.json"))
    args = ap.parse_args()
    chains = [c for i in range(args.complexes) for c in synth.synthetic_complex(1000 + i, args.residues, args.residues)]
    gb = build_graph_batch(chains, k=20)
    record = {"shape": {"complexes": args.complexes, "residues": args.residues, "k": 20, "nodes": gb.num_nodes,
                        "edges": gb.num_edges, "geo_ref": bool(gb.geo_ref)},
              "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "warmup": args.warmup,
              "unit": "ms per forward, median over rounds (min, max)", "dtypes": {}}
    ok = True
    for dtype in ("bf16", "f32"):
        engines = {}
        for mode, plain in (("plain", True), ("geometric", False)):
            cfg = GeoTConfig(disable_geometric_mode=plain)
            engines[mode] = GeoTEngine(seeded_state_dict(0, cfg, with_head=False), dtype, cfg)
        for eng in engines.values():
            for _ in range(args.warmup):
                one_forward(eng, gb)
        rounds = {mode: [] for mode in engines}
        for _ in range(args.rounds):
            for mode, eng in engines.items():
                rounds[mode].append(one_forward(eng, gb))
        out = {}
        for mode, rs in rounds.items():
            names = sorted(rs[0])
            kern = {n: [round(f([r[n] for r in rs]), 4) for f in (statistics.median, min, max)] for n in names}
            edge = [r.get("edge_layer", 0.0) + r["edge_layer_final"] for r in rs]
            total = [sum(r.values()) for r in rs]
            out[mode] = {"kernels": kern, "edge_ms": [round(f(edge), 4) for f in (statistics.median, min, max)],
                         "total_ms": [round(f(total), 4) for f in (statistics.median, min, max)]}
        out["plain_edge_le_geometric"] = out["plain"]["edge_ms"][0] <= out["geometric"]["edge_ms"][0]
        ok = ok and out["plain_edge_le_geometric"]
        record["dtypes"][dtype] = out
        print(dtype, json.dumps(out))
        del engines
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
