"""Scoring a prediction from structures on the GPU: LitGINI.test_batch_structures and
test_sharded(structures=...) against the same calls fed example lists that were built on the host from
tests/interface_cases.ref_labels_f32 of the same structures. The label maps are then equal byte for byte
(tests/test_gpu_interface.py), everything behind them is one code path, so every key of every dict must be
equal to the bit."""
import os

import numpy as np
import pytest
import torch

import interface_cases as ic
from test_gpu_c4 import _model

pytestmark = pytest.mark.gpu

SIZES = [(24, 31), (40, 22), (21, 21)]
SEED = 5
FILEPATHS = [os.path.join("data", "final", f"{chr(97 + i)}{i}xy_complex.dill") for i in range(len(SIZES))]


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape \
            and a.tobytes() == b.tobytes()
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    return a == b and type(a) is type(b)


@pytest.fixture(scope="module")
def setup():
    from deepinteract_amd import synth
    from deepinteract_amd.builder import build_graph_batch
    model = _model()
    cx = [synth.synthetic_complex(300 + i, a, b) for i, (a, b) in enumerate(SIZES)]
    structures = [ic.structure_for(a, b, 20 + i) for i, (a, b) in enumerate(SIZES)]
    labels = [ic.ref_labels_f32(*s) for s in structures]
    assert all(lab.sum() > 0 for lab in labels)
    examples = [torch.from_numpy(ic.examples_from_labels(lab, a, b)) for lab, (a, b) in zip(labels, SIZES)]
    gb = build_graph_batch([c for pair in cx for c in pair], k=20, device="cuda:0",
                           node_count_limit=model.cfg.node_count_limit,
                           nbr_seeds=[SEED + 2 * i + s for i in range(len(cx)) for s in (0, 1)])
    pairs = [(2 * j, 2 * j + 1) for j in range(len(cx))]
    return model, cx, structures, labels, examples, gb, pairs


def test_test_batch_structures_equals_test_batch_on_host_built_lists(setup):
    model, _, structures, labels, examples, gb, pairs = setup
    with torch.no_grad():
        want = model.test_batch(gb, pairs, examples, FILEPATHS)
        got = model.test_batch_structures(gb, pairs, structures, FILEPATHS)
        got_keep1 = model.test_batch_structures(gb, pairs, structures, FILEPATHS, keep_maps=1)
    assert len(got) == len(want) == len(SIZES)
    for c, (g, w, lab) in enumerate(zip(got, want, labels)):
        assert set(g) == set(w)
        for key in w:
            assert _same(g[key], w[key]), (c, key, g[key], w[key])
        assert g["test_labels"].tobytes() == lab.astype(np.float32).tobytes()
        assert g["confusion"]["tp"] + g["confusion"]["fn"] == int(lab.sum())
    for c, (g, w) in enumerate(zip(got_keep1, want)):
        for key in w:
            if key in ("test_preds", "test_preds_rounded", "test_labels") and c >= 1:
                assert g[key] is None
            else:
                assert _same(g[key], w[key]), (c, key)


def test_another_cutoff_reaches_the_labels(setup):
    model, _, structures, _, _, gb, pairs = setup
    with torch.no_grad():
        got = model.test_batch_structures(gb, pairs, structures, FILEPATHS, cutoff=4.5)
    for g, s in zip(got, structures):
        assert g["test_labels"].tobytes() == ic.ref_labels_f32(*s, cutoff=4.5).astype(np.float32).tobytes()


def test_a_residue_count_mismatch_raises_before_any_launch(setup):
    model, _, structures, _, _, gb, pairs = setup
    calls = []
    forward = model._forward_batch
    model._forward_batch = lambda *a, **k: calls.append(1) or forward(*a, **k)
    try:
        (x0, o0), c1 = structures[1]
        short = ((x0[:o0[-2]], o0[:-1]), c1)                  # chain 0 one residue short
        with pytest.raises(ValueError, match="residues"):
            model.test_batch_structures(gb, pairs, [structures[0], short, structures[2]], FILEPATHS)
        with pytest.raises(ValueError, match="residues"):
            model.test_batch_structures(gb, pairs, [structures[0], (structures[1][1], structures[1][0]),
                                                    structures[2]], FILEPATHS)
        with pytest.raises(ValueError, match="one structure and one file path"):
            model.test_batch_structures(gb, pairs, structures[:2], FILEPATHS)
    finally:
        model._forward_batch = forward
    assert calls == []


def test_test_sharded_from_structures_equals_from_examples(setup, tmp_path):
    import torch.distributed as dist
    from deepinteract_amd.distributed import test_sharded
    model, cx, structures, _, examples, _, _ = setup
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        kw = dict(micro_batch=2, k=20, seed=SEED, device="cuda:0")
        want = test_sharded(model, cx, examples, FILEPATHS, **kw)
        got = test_sharded(model, cx, None, FILEPATHS, structures=structures, **kw)
        via_model = model.test_sharded(cx, None, FILEPATHS, structures=structures, **kw)
        for name, outs in (("function", got), ("method", via_model)):
            assert len(outs) == len(want) == len(SIZES)
            for c, (g, w) in enumerate(zip(outs, want)):
                assert _same(g, w), (name, c, [k for k in w if not _same(g.get(k), w[k])])
        with pytest.raises(ValueError, match="exactly one of"):
            test_sharded(model, cx, examples, FILEPATHS, structures=structures, **kw)
        with pytest.raises(ValueError, match="exactly one of"):
            test_sharded(model, cx, None, FILEPATHS, **kw)
        with pytest.raises(ValueError, match="residues"):
            test_sharded(model, cx, None, FILEPATHS, structures=[structures[0], structures[0], structures[2]], **kw)
    finally:
        dist.destroy_process_group()
