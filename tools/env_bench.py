"""Residue-environment benchmark (outside the metric): structure.ResidueEnvOp.features (one memset and three
launches for all chains, csrc/residue_env.hip) from device tensors and from host arrays, against three
other ways to the same columns (HSAAC, CN; compared here with the op's):

  kdtree_host        the sensible CPU way: scipy's cKDTree over the fp64 atoms (query_pairs at sqrt(c2)),
                     residue neighbours as a sparse set, the half-sphere counts with numpy
  reference_loop     the reference's shape (get_similarity_matrix, dips_plus_utils.py:84-115): a Python double
                     loop over residue pairs with one scipy cdist per pair, then the same numpy epilogue;
                     at the smallest shape only
  torch_device       dense torch on the device, inputs already there: the [A, A] squared distances by
                     broadcast differences in row slices of at most 2^26 elements, a segmented any() per
                     residue pair (two index_add_ passes), side-chain vectors by index_add_, the counts as
                     [L, L] x [L, 21] matmuls

Inputs: synthetic full-atom chains, seeded: a CA random walk with 3.8 A steps pulled towards the origin,
4-14 atoms per residue (N, CA, C, O 1.5 A from CA, a CB and other side atoms around a point 2.5 A away).
Shapes: 16 x 145, 16 x 256, 2 x 1000, 1 x 4000 residues.

Timing: a host clock around calls that end in a device synchronise (the op ends with its host read of the
flags; torch_device is followed by torch.cuda.synchronize()). Every side is warmed up, then the sides are
timed in alternating windows; the median window is reported with the fastest and slowest (ms per call over
all chains of the shape). Needs a GPU: there is no CPU path.

usage: python tools/env_bench.py [--windows 5] [--out profiles/residue_env_bench.json]
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

CASES = ((16, 145), (16, 256), (2, 1000), (1, 4000))
REPS = {"op_device": 10, "op_host": 10, "torch_device": 2, "kdtree_host": 1, "reference_loop": 1}
SLICE = 1 << 26


def synthetic_chain(rng, L):
    """(xyz f32 [A, 3], res_off i32 [L + 1], role u8 [A], aa u8 [L], resname_idx u8 [L])."""
    ca = np.zeros((L, 3))
    for i in range(1, L):
        step = rng.normal(size=3) - 0.01 * ca[i - 1]
        ca[i] = ca[i - 1] + 3.8 * step / np.linalg.norm(step)
    counts = rng.integers(4, 15, size=L)
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    xyz = np.repeat(ca + 2.5 * unit(rng.normal(size=(L, 3))), counts, axis=0) + rng.normal(scale=0.9, size=(off[-1], 3))
    role = np.zeros(off[-1], dtype=np.uint8)
    for q, code in enumerate((1, 2, 3, 4)):                    # N, CA, C, O first
        xyz[off[:-1] + q] = ca if code == 2 else ca + 1.5 * unit(rng.normal(size=(L, 3)))
        role[off[:-1] + q] = code
    has_cb = counts > 4
    role[off[:-1][has_cb] + 4] = 5
    aa = rng.integers(0, 21, size=L).astype(np.uint8)
    col = np.minimum(aa, 19).astype(np.uint8)                  # any valid column: the timing does not depend on it
    return np.ascontiguousarray(xyz, dtype=np.float32), off, role, aa, col


def side_vectors(chain):
    """(ca [L, 3], u [L, 3]) in fp64, numpy."""
    xyz, off, role = chain[0].astype(np.float64), chain[1], chain[2]
    L = len(off) - 1
    res = np.repeat(np.arange(L), np.diff(off))
    pos = {q: np.zeros((L, 3)) for q in (1, 2, 3)}
    for q in pos:
        pos[q][res[role == q]] = xyz[role == q]
    ca = pos[2]
    side = (role == 0) | (role == 5)
    v = xyz[side] - ca[res[side]]
    u = np.zeros((L, 3))
    np.add.at(u, res[side], v / np.linalg.norm(v, axis=1, keepdims=True))
    n = np.bincount(res[side], minlength=L)
    gly = n == 0

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    u[~gly] /= n[~gly, None]
    u[gly] = 0.5 * (unit(ca[gly] - pos[3][gly]) + unit(ca[gly] - pos[1][gly]))
    return ca, u


def epilogue(nb, chain):
    """(cn_raw [L], hsaac [L, 42] fp32) from a dense boolean neighbour matrix (diagonal set), numpy."""
    aa = chain[3]
    L = len(aa)
    ca, u = side_vectors(chain)
    dots = ((ca[None] - ca[:, None]) * u[:, None]).sum(axis=2)
    up = nb & ~np.eye(L, dtype=bool) & (dots > 0)
    down = nb & ~up
    kind = np.eye(21)[aa]
    num = np.concatenate((up @ kind + kind, down @ kind + kind), axis=1)
    den = np.concatenate((np.repeat(1.0 + up.sum(1)[:, None], 21, 1), np.repeat(1.0 + down.sum(1)[:, None], 21, 1)), 1)
    return nb.sum(axis=1).astype(np.int32), (num / den).astype(np.float32)


def kdtree_features(chain, c2):
    from scipy.spatial import cKDTree
    xyz, off = chain[0].astype(np.float64), chain[1]
    L = len(off) - 1
    res = np.repeat(np.arange(L), np.diff(off))
    pairs = cKDTree(xyz).query_pairs(float(np.sqrt(c2)), output_type="ndarray")
    nb = np.eye(L, dtype=bool)
    nb[res[pairs[:, 0]], res[pairs[:, 1]]] = True
    nb |= nb.T
    return epilogue(nb, chain)


def reference_loop_features(chain, c2):
    from scipy.spatial.distance import cdist
    xyz, off = chain[0].astype(np.float64), chain[1]
    L = len(off) - 1
    coords = [xyz[off[i]:off[i + 1]] for i in range(L)]
    nb = np.eye(L, dtype=bool)
    for i in range(L):
        for j in range(i + 1, L):
            if cdist(coords[i], coords[j]).min() ** 2 < c2:
                nb[i, j] = nb[j, i] = True
    return epilogue(nb, chain)


def torch_features(chain, c2):
    """The dense device version for one chain of device tensors -> (cn_raw int32 [L], hsaac fp32 [L, 42])."""
    xyz, off, role, aa, _ = chain
    L, A = aa.numel(), xyz.shape[0]
    dev = xyz.device
    res = torch.repeat_interleave(torch.arange(L, device=dev), (off[1:] - off[:-1]).long())
    rows = max(1, SLICE // A)
    hit_rows = torch.zeros(L, A, device=dev)
    for a in range(0, A, rows):
        dx, dy, dz = (xyz[a:a + rows, c:c + 1] - xyz[:, c][None, :] for c in range(3))
        hit = (((dx * dx + dy * dy) + dz * dz) < c2).float()
        hit_rows.index_add_(0, res[a:a + rows], hit)
    nb = torch.zeros(L, L, device=dev).index_add_(1, res, (hit_rows > 0).float()) > 0
    nb.fill_diagonal_(True)
    pos = {}
    for q in (1, 2, 3):
        pos[q] = torch.zeros(L, 3, device=dev).index_copy_(0, res[role == q], xyz[role == q])
    ca = pos[2]
    side = (role == 0) | (role == 5)
    v = xyz[side] - ca[res[side]]
    u = torch.zeros(L, 3, device=dev).index_add_(0, res[side], v / v.norm(dim=1, keepdim=True))
    n = torch.zeros(L, device=dev).index_add_(0, res[side], torch.ones(int(side.sum()), device=dev))
    gly = 0.5 * ((ca - pos[3]) / (ca - pos[3]).norm(dim=1, keepdim=True) + (ca - pos[1]) / (ca - pos[1]).norm(dim=1, keepdim=True))
    u = torch.where((n > 0)[:, None], u / n.clamp(min=1)[:, None], gly)
    dots = (ca @ u.T).T - (ca * u).sum(dim=1)[:, None]          # dots[i, j] = u_i . (ca_j - ca_i)
    up = nb & (dots > 0)
    up.fill_diagonal_(False)
    down = nb & ~up
    kind = torch.nn.functional.one_hot(aa.long(), 21).float()
    num = torch.cat((up.float() @ kind + kind, down.float() @ kind + kind), dim=1)
    den = torch.cat(((1 + up.sum(1))[:, None].expand(L, 21), (1 + down.sum(1))[:, None].expand(L, 21)), dim=1)
    return nb.sum(dim=1).to(torch.int32), num / den


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residue_env_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("env_bench needs a ROCm GPU")
    from deepinteract_amd.structure import ENV_C2, ResidueEnvOp
    op = ResidueEnvOp("cuda")
    rng = np.random.default_rng(2025)
    rows = []
    for k, (count, L) in enumerate(CASES):
        host = [synthetic_chain(rng, L) for _ in range(count)]
        dev = [tuple(torch.from_numpy(x).cuda() for x in c) for c in host]

        def op_device():
            return op.features(dev)

        def op_host():
            return op.features(host)

        def torch_device():
            return [torch_features(c, ENV_C2) for c in dev]

        def kdtree_host():
            return [kdtree_features(c, ENV_C2) for c in host]

        def reference_loop():
            return [reference_loop_features(c, ENV_C2) for c in host]

        sides = {"op_device": op_device, "op_host": op_host, "torch_device": torch_device, "kdtree_host": kdtree_host}
        if k == 0:
            sides["reference_loop"] = reference_loop
        want = [(r["cn_raw"].cpu().numpy(), r["dips"][:, 36:78].cpu().numpy()) for r in op_device()]
        same = {}
        for name in ("op_host", "torch_device", "kdtree_host", "reference_loop"):
            if name not in sides:
                continue
            got = sides[name]()
            if name == "op_host":
                got = [(r["cn_raw"], r["dips"][:, 36:78]) for r in got]
            got = [tuple(x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in g) for g in got]
            same[name] = {"cn_raw": all(np.array_equal(g[0], w[0]) for g, w in zip(got, want)),
                          "hsaac": all(np.array_equal(g[1], w[1]) for g, w in zip(got, want))}
        t = measure(sides, a.windows)
        cn = np.concatenate([w[0] for w in want])
        row = {"chains": count, "residues": L, "atoms": int(sum(c[0].shape[0] for c in host)),
               "cn_min_mean_max": [int(cn.min()), float(cn.mean()), int(cn.max())], "equal_to_op_device": same,
               "times": t, "torch_device_over_op_device": t["torch_device"]["ms"] / t["op_device"]["ms"],
               "kdtree_host_over_op_host": t["kdtree_host"]["ms"] / t["op_host"]["ms"]}
        if "reference_loop" in t:
            row["reference_loop_over_op_host"] = t["reference_loop"]["ms"] / t["op_host"]["ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
    out = {"workload": "structure-derived DIPS-Plus columns (one-hot, HSAAC, CN) and amide normals of ragged batches "
                       "of chains: ResidueEnvOp vs dense torch on the device vs cKDTree vs the reference's pair loop",
           "device": torch.cuda.get_device_name(0), "windows": a.windows, "c2": ENV_C2, "seed": 2025,
           "timing": "host clock around calls that end in a device synchronise, median window, ms per call over "
                     "all chains of the shape",
           "results": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
