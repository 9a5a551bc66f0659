"""Interface-label benchmark (outside the metric): ranking.InterfaceOp.labels (one memset and two launches
for all complexes, csrc/contact_interface.hip) from host arrays and from device tensors, against the
two routes it replaces, all producing the same maps (checked here):

  (a) device torch   per complex the [A0, A1] atom-pair mask and the per-residue reductions as two
                     index_add_ passes; inputs already on the device. The mask comes from torch.cdist in
                     its exact mode (no matmul; it launches one block per atom pair, so chain 0's atoms
                     go through it in slices of at most 2^23 pairs, below the launch limit) <= cutoff
                     ("torch_cdist"), or from broadcast elementwise differences, (dx * dx + dy * dy) +
                     dz * dz <= cutoff^2 ("torch_elementwise"): both times are reported
  (b) today's path   labels on the host with scipy's cKDTree, the reference's complete [L1 * L2, 3] int64
                     example list built and copied to the device, ExamplesOp.labels

Inputs: synthetic bound pairs, seeded. Each chain is a CA random walk with 3.8 A steps whose z is folded
to one side of a plane, so the two chains lie face to face 4 A apart; 4-14 atoms per residue, jittered
around the CA (sigma 1.2 A). Shapes: 16 x 256^2, 2 x 1000^2, 1 x 4000^2 residues. The positive share of
every case is recorded.

Timing: a host clock around calls that end in a device synchronise (the op's and route (b)'s calls end
with their host read of the flags; route (a) is followed by torch.cuda.synchronize()), because routes
(b) and "from host arrays" are mostly host work. Every side is warmed up, then the sides are timed in
alternating windows and the median window is reported with the fastest and slowest (ms per call over the
whole set of complexes). Needs a GPU: there is no CPU path.

usage: python tools/interface_bench.py [--windows 5] [--out profiles/interface_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((16, 256), (2, 1000), (1, 4000))
CUTOFF = 6.0
REPS = {"op_host": 10, "op_device": 10, "torch_cdist": 2, "torch_elementwise": 3, "kdtree_examples": 1}
CDIST_PAIRS = 1 << 23      # atom pairs per torch.cdist call: one block of 256 threads each, below 2^32 threads


def bound_pair(rng, l1, l2):
    """((xyz0, res_off0), (xyz1, res_off1)) of one synthetic complex."""
    out = []
    for s, l in enumerate((l1, l2)):
        step = rng.normal(size=(l, 3))
        ca = np.cumsum(3.8 * step / np.linalg.norm(step, axis=1, keepdims=True), axis=0)
        ca[:, 2] = np.abs(ca[:, 2]) + 4.0 if s else -np.abs(ca[:, 2])
        counts = rng.integers(4, 15, size=l)
        xyz = np.repeat(ca, counts, axis=0) + rng.normal(scale=1.2, size=(counts.sum(), 3))
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        out.append((np.ascontiguousarray(xyz, dtype=np.float32), off))
    return tuple(out)


def torch_labels(c0, c1, cutoff=CUTOFF, cdist=True):
    """Route (a) for one complex: c? = (xyz [A, 3] fp32, res_off [L + 1] int32) tensors on one device."""
    (x0, o0), (x1, o1) = c0, c1
    l1, l2 = o0.numel() - 1, o1.numel() - 1
    res0 = torch.repeat_interleave(torch.arange(l1, device=x0.device), (o0[1:] - o0[:-1]).long())
    res1 = torch.repeat_interleave(torch.arange(l2, device=x1.device), (o1[1:] - o1[:-1]).long())
    if cdist:
        rows = max(1, CDIST_PAIRS // x1.shape[0])
        hit = torch.cat([torch.cdist(x0[a:a + rows], x1, compute_mode="donot_use_mm_for_euclid_dist") <= cutoff
                         for a in range(0, x0.shape[0], rows)]).float()
    else:
        dx, dy, dz = (x0[:, c:c + 1] - x1[:, c][None, :] for c in range(3))
        hit = (((dx * dx + dy * dy) + dz * dz) <= float(np.float32(cutoff * cutoff))).float()
    rows = torch.zeros(l1, x1.shape[0], device=x0.device).index_add_(0, res0, hit) > 0
    both = torch.zeros(l1, l2, device=x0.device).index_add_(1, res1, rows.float()) > 0
    return both.to(torch.uint8).view(-1)


def kdtree_examples(c0, c1, cutoff=CUTOFF):
    """Route (b)'s host half for one complex: the complete [L1 * L2, 3] int64 example list, as the
    reference's build_examples_tensor lays it out, with the labels cKDTree gives."""
    from scipy.spatial import cKDTree
    (x0, o0), (x1, o1) = c0, c1
    l1, l2 = len(o0) - 1, len(o1) - 1
    res0 = np.repeat(np.arange(l1), np.diff(o0))
    res1 = np.repeat(np.arange(l2), np.diff(o1))
    pairs = cKDTree(x0.astype(np.float64)).query_ball_tree(cKDTree(x1.astype(np.float64)), r=cutoff)
    lab = np.zeros((l1, l2), dtype=np.int64)
    for a, hits in enumerate(pairs):
        if hits:
            lab[res0[a], res1[hits]] = 1
    i, j = np.divmod(np.arange(l1 * l2, dtype=np.int64), l2)
    return np.stack((i, j, lab.reshape(-1)), axis=1)


def window(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def measure(sides, windows):
    for name, fn in sides.items():      # warm-up: code objects, allocator, pinned pool
        for _ in range(2 if REPS[name] > 1 else 1):
            fn()
    times = {name: [] for name in sides}
    for _ in range(windows):
        for name, fn in sides.items():
            times[name].append(window(fn, REPS[name]))
    return {name: {"ms": statistics.median(t), "ms_min_max": [min(t), max(t)], "reps_per_window": REPS[name]}
            for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interface_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interface_bench needs a ROCm GPU")
    from deepinteract_amd.ranking import ExamplesOp, InterfaceOp
    op, ex_op = InterfaceOp("cuda"), ExamplesOp("cuda")
    rng = np.random.default_rng(2024)
    rows, unequal = [], []
    for count, side in CASES:
        host = [bound_pair(rng, side, side) for _ in range(count)]
        dev = [tuple((torch.from_numpy(x).cuda(), torch.from_numpy(o).cuda()) for x, o in c) for c in host]
        shapes = [(side, side)] * count

        def op_host():
            return op.labels([c[0] for c in host], [c[1] for c in host], cutoff=CUTOFF)

        def op_device():
            return op.labels([c[0] for c in dev], [c[1] for c in dev], cutoff=CUTOFF)

        def torch_cdist():
            return [torch_labels(c0, c1) for c0, c1 in dev]

        def torch_elementwise():
            return [torch_labels(c0, c1, cdist=False) for c0, c1 in dev]

        def kdtree():
            lists = [torch.from_numpy(kdtree_examples(c0, c1)).cuda() for c0, c1 in host]
            return ex_op.labels(lists, shapes)

        want = [m.clone() for m in op_host()]
        num_pos = list(op.num_pos)
        same = {"op_device": all(torch.equal(x, y) for x, y in zip(op_device(), want)),
                "torch_cdist": all(torch.equal(x, y) for x, y in zip(torch_cdist(), want)),
                "torch_elementwise": all(torch.equal(x, y) for x, y in zip(torch_elementwise(), want)),
                "kdtree_examples": all(torch.equal(x, y) for x, y in zip(kdtree(), want))}
        unequal += [f"{count} x {side}^2: {k}" for k, v in same.items() if not v]
        t = measure({"op_host": op_host, "op_device": op_device, "torch_cdist": torch_cdist,
                     "torch_elementwise": torch_elementwise, "kdtree_examples": kdtree}, a.windows)
        row = {"complexes": count, "shape": [side, side], "atoms": int(sum(len(c[0][0]) + len(c[1][0]) for c in host)),
               "positives": int(sum(num_pos)), "positives_share": sum(num_pos) / (count * side * side),
               "equal_maps": same, "times": t,
               "torch_cdist_over_op_device": t["torch_cdist"]["ms"] / t["op_device"]["ms"],
               "torch_elementwise_over_op_device": t["torch_elementwise"]["ms"] / t["op_device"]["ms"],
               "kdtree_examples_over_op_host": t["kdtree_examples"]["ms"] / t["op_host"]["ms"],
               "example_list_bytes": 24 * count * side * side, "atom_bytes": int(sum(c[s][0].nbytes + c[s][1].nbytes
                                                                                    for c in host for s in (0, 1)))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
    out = {"workload": "label maps of bound complexes from heavy-atom coordinates: InterfaceOp vs torch.cdist on the "
                       "device vs cKDTree + example lists + ExamplesOp",
           "device": torch.cuda.get_device_name(0), "windows": a.windows, "cutoff": CUTOFF, "seed": 2024,
           "timing": "host clock around calls that end in a device synchronise, median window, ms per call over "
                     "all complexes",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    if unequal:
        raise SystemExit("maps differ from InterfaceOp's: " + "; ".join(unequal))


if __name__ == "__main__":
    main()
