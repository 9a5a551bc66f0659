"""bench.py --dump-outputs on a small shape: a plain run (no --full) writes the arrays the timed
schedule's last micro-batch left in HBM, the same bytes in every run, and they are what the engine
and the pair-tensor definition give for that micro-batch:
* node_feats / edge_feats == GeoTEngine.forward of the same device-built micro-batch computed alone
  (the kernels are deterministic: bit-identical), node_feats_T its transpose;
* pair_tensor == the outer concat of those node features (construct_interact_tensor), every element.
Two micro-batches per step and --pool 4, so the two rotating sinks hold different complexes and the
last job's sink is the second one."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N_RES, K, POOL, CX = 2, 64, 20, 4, 4
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--complexes", str(CX), "--micro-batch", str(M),
        "--residues", str(N_RES), "--knn", str(K), "--pool", str(POOL)]
NAMES = ("node_feats", "edge_feats", "node_feats_T", "pair_tensor")


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    import bench
    out = []
    for tag in ("a", "b"):
        d = str(tmp_path_factory.mktemp("dump_" + tag))
        line = bench.main(ARGS + ["--dump-outputs", d])
        out.append((d, line, {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}))
    return out


def test_plain_line_and_files(dumps):
    d, line, arrs = dumps[0]
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    assert all(a.dtype == np.float32 for a in arrs.values())
    json.dumps(line)
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "bf16" and line["unit"] == "complexes/s"
    assert abs(line["value"] - CX * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    # a plain run measures nothing beside the timed steps
    assert "cpu_baseline" not in line and "sub_records" not in line and "head_prologue" not in line
    assert set(line["kernels"]) <= {"pair_tensor"} and line["host_issue_ms_per_step"] is None


def test_same_bytes_every_run(dumps):
    for n in NAMES:
        assert np.array_equal(dumps[0][2][n], dumps[1][2][n]), n


def test_dump_is_the_last_micro_batch(dumps):
    from deepinteract_amd import synth
    from deepinteract_amd.builder import build_graph_batch
    from deepinteract_amd.engine import GeoTEngine
    from deepinteract_amd.graph import select_graphs
    from deepinteract_amd.weights import seeded_state_dict

    arrs = dumps[0][2]
    # the bench's inputs: pool complex c from synth seed c, neighbour seeds 2c + s + 1; the last of the
    # CX / M micro-batches holds complexes ((CX / M - 1) * M + j) % POOL
    chains = [ch for c in range(POOL) for ch in synth.synthetic_complex(c, N_RES, N_RES)]
    pool = build_graph_batch(chains, k=K, device=torch.device("cuda", 0), node_count_limit=2304,
                             nbr_seeds=[2 * c + s + 1 for c in range(POOL) for s in (0, 1)])
    m = CX // M - 1
    gb = select_graphs(pool, [2 * ((m * M + j) % POOL) + s for j in range(M) for s in (0, 1)])
    eng = GeoTEngine(seeded_state_dict(0, with_head=False), "bf16", device=torch.device("cuda", 0))
    eng.fuse_embed_init, eng.split_node, eng.resident_init = True, False, False  # bench.py's overlapped defaults
    h, e = eng.forward(gb)
    torch.cuda.synchronize()
    h, e = h.float().cpu().numpy(), e.float().cpu().numpy()
    assert h.shape == (2 * M * N_RES, 128) and np.isfinite(h).all() and np.abs(h).max() > 0
    assert np.array_equal(arrs["node_feats"], h)
    assert np.array_equal(arrs["edge_feats"], e)
    assert np.array_equal(arrs["node_feats_T"], h.T)
    pair = arrs["pair_tensor"].reshape(M, 256, N_RES, N_RES)
    for j in range(M):
        a, b = h[gb.node_off[2 * j]:gb.node_off[2 * j] + N_RES], h[gb.node_off[2 * j + 1]:gb.node_off[2 * j + 1] + N_RES]
        assert np.array_equal(pair[j, :128], np.broadcast_to(a.T[:, :, None], (128, N_RES, N_RES))), j
        assert np.array_equal(pair[j, 128:], np.broadcast_to(b.T[:, None, :], (128, N_RES, N_RES))), j

