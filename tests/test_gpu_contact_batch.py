"""Batched contact ranking / AUC on the GPU (di_contact_rank_batch, di_contact_auc_batch,
ranking.ContactRankOp.batch / ContactAucOp.batch, LitGINI.test_batch / test_epoch_end).

The contract: a block of a batched launch runs the single call's kernel body on the single call's
geometry, so every output of every complex EQUALS the single op's on the same inputs, bit for bit
(ce_sum, auroc and auprc included), whatever its neighbours in the batch hold. The single ops are
guarded by test_gpu_contact_rank.py / test_gpu_contact_auc.py; two complexes are compared against
those modules' independent yardsticks here too, with their bounds."""
import math
import struct

import numpy as np
import pytest
import torch

from gpu_common import load_case
from test_gpu_contact_auc import against_ref, _residue_graph
from test_gpu_contact_rank import check_order

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from deepinteract_amd.ranking import ContactAucOp, ContactRankOp
    return ContactRankOp("cuda"), ContactAucOp("cuda")


def bernoulli(n, share, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) < share).to(torch.uint8)


def exactly(n, num_pos, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(n, dtype=torch.uint8)
    lab[torch.randperm(n, generator=g)[:num_pos]] = 1
    return lab


def randn_logits(l1, l2, seed, scale=6.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(1, 2, l1, l2, generator=g)


def _cases():
    """(name, fp32 logits [1, 2, L1, L2], uint8 labels [n], k or None) on the host."""
    out = [("1x1", randn_logits(1, 1, 1), torch.ones(1, dtype=torch.uint8), 1),
           ("3x5, K = n", randn_logits(3, 5, 2), bernoulli(15, 0.3, 3), 15)]
    c1 = torch.as_tensor(load_case("c1")["logits"]).float().contiguous()
    assert c1.shape[2] * c1.shape[3] % 2 == 1
    out.append(("c1 145x145", c1, bernoulli(c1.shape[2] * c1.shape[3], 0.01, 4), None))
    out.append(("7x400", randn_logits(7, 400, 5), bernoulli(2800, 0.01, 6), None))
    out.append(("256x257 all equal", torch.full((1, 2, 256, 257), 0.25), bernoulli(256 * 257, 0.01, 7), 256))
    g = torch.Generator().manual_seed(8)
    n = 300 * 300
    l1 = torch.full((n,), -1.0)
    l1[torch.randperm(n, generator=g)[:100]] = 3.0           # 100 high, the rest one tie group across K = 256
    out.append(("300x300 tie group across K", torch.stack((torch.zeros(n), l1)).view(1, 2, 300, 300).contiguous(),
                bernoulli(n, 0.01, 9), 256))
    out.append(("300x300 P = 4096", randn_logits(300, 300, 10, 2.0), exactly(n, 4096, 11), None))
    out.append(("300x300 P = 4097", randn_logits(300, 300, 12, 2.0), exactly(n, 4097, 13), None))
    nan = randn_logits(64, 65, 14)
    nan.view(2, -1)[0, 17] = nan.view(2, -1)[1, 900] = nan.view(2, -1)[1, 4159] = float("nan")
    out.append(("64x65 three NaN", nan, bernoulli(64 * 65, 0.05, 15), None))
    out.append(("50x70 no positives", randn_logits(50, 70, 16), torch.zeros(3500, dtype=torch.uint8), None))
    out.append(("200x200 saturated", randn_logits(200, 200, 17, 30.0), bernoulli(40000, 0.02, 18), None))
    return out


def _bits(m):
    return {k: struct.pack("d", v) if isinstance(v, float) else v for k, v in m.items()}


def record(r, a):
    """Everything a complex's results hold, as comparable host values (floats by their bits)."""
    torch.cuda.synchronize()
    return {"probs": r.probs.cpu().numpy().tobytes(), "shape": tuple(r.probs.shape), "ids": r.ids.cpu().tolist(),
            "scores": r.scores.cpu().numpy().tobytes(), "hits": r.hits.cpu().tolist(), "rank": _bits(r.metrics()),
            "auc": _bits(a.metrics())}


_cache = {}


def prepared(ops, dtype):
    """The cases on the device in `dtype`, with the single ops' records: computed once per dtype."""
    if dtype not in _cache:
        rank, auc = ops
        cases = [(name, lg.to(dtype).cuda().contiguous(), lab.cuda(), k) for name, lg, lab, k in _cases()]
        refs = []
        for name, lg, lab, k in cases:
            r = rank(lg, k=k, labels=lab)
            refs.append(record(r, auc(r.probs, lab)))
        _cache[dtype] = (cases, refs)
    return _cache[dtype]


def run_batch(ops, cases, max_pos=None):
    rank, auc = ops
    rs = rank.batch([c[1] for c in cases], k=[c[3] for c in cases], labels_list=[c[2] for c in cases])
    aus = auc.batch([r.probs for r in rs], [c[2] for c in cases], max_pos=max_pos)
    return rs, aus


def assert_same(got, want, what):
    for key in want:
        assert got[key] == want[key], (what, key, got[key] if key in ("rank", "auc", "shape") else "...",
                                       want[key] if key in ("rank", "auc", "shape") else "...")


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_batch_equals_single_ops(ops, dtype):
    cases, refs = prepared(ops, dtype)
    rs, aus = run_batch(ops, cases)
    assert len(rs) == len(aus) == len(cases) == 11
    for (name, lg, lab, k), r, a, ref in zip(cases, rs, aus, refs):
        assert r.probs.data_ptr() % 16 == 0 and r.probs.is_contiguous()
        assert_same(record(r, a), ref, f"{name} {dtype}")
    # what the cases are there for
    by = {c[0]: ref for c, ref in zip(cases, refs)}
    assert by["300x300 P = 4096"]["auc"]["num_pos"] == 4096 and by["300x300 P = 4097"]["auc"]["num_pos"] == 4097
    assert by["64x65 three NaN"]["auc"]["num_nan"] == 3
    assert math.isnan(struct.unpack("d", by["64x65 three NaN"]["auc"]["auroc"])[0])
    assert by["50x70 no positives"]["rank"]["num_pos"] == 0
    assert math.isnan(struct.unpack("d", by["50x70 no positives"]["auc"]["auroc"])[0])
    assert by["256x257 all equal"]["ids"] == list(range(256))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reverse_order_gives_the_same_bits(ops, dtype):
    cases, refs = prepared(ops, dtype)
    rs, aus = run_batch(ops, cases[::-1])
    for (name, *_), r, a, ref in zip(cases[::-1], rs, aus, refs[::-1]):
        assert_same(record(r, a), ref, f"{name} {dtype} reversed")


@pytest.mark.parametrize("dtype", DTYPES)
def test_independent_yardsticks(ops, dtype):
    """torch.sort(stable) of the stored map and ref_auc, with the single ops' tests' bounds."""
    cases, _ = prepared(ops, dtype)
    picked = [c for c in cases if c[0] in ("c1 145x145", "300x300 P = 4097")]
    assert len(picked) == 2
    rs, aus = run_batch(ops, picked)
    torch.cuda.synchronize()
    for (name, lg, lab, _), r, a in zip(picked, rs, aus):
        check_order(r, r.ids.numel())
        hits = torch.cumsum(lab[r.ids.long()].long(), 0)
        assert torch.equal(r.hits.long(), hits)
        against_ref(a, r.probs, lab, f"batched {name} {dtype}")


def test_count_one(ops):
    cases, refs = prepared(ops, torch.float32)
    for i in (2, 7):
        rs, aus = run_batch(ops, cases[i:i + 1])
        assert len(rs) == 1
        assert_same(record(rs[0], aus[0]), refs[i], cases[i][0])


def test_seventy_small_distinct_maps(ops):
    """More complexes than a block has waves, and more than 64."""
    rank, auc = ops
    cases = []
    for i in range(70):
        l1, l2 = 3 + i % 5, 4 + i % 7
        cases.append((f"small {i}", randn_logits(l1, l2, 100 + i).cuda(), bernoulli(l1 * l2, 0.3, 200 + i).cuda(), None))
    rs, aus = run_batch(ops, cases)
    got = [record(r, a) for r, a in zip(rs, aus)]
    for (name, lg, lab, k), g in zip(cases, got):
        r = rank(lg, k=k, labels=lab)
        assert_same(g, record(r, auc(r.probs, lab)), name)
    assert len({g["probs"] for g in got}) == 70


def test_two_batches_back_to_back_without_a_host_sync(ops):
    cases, refs = prepared(ops, torch.float32)
    first = run_batch(ops, cases[:5])
    second = run_batch(ops, cases[5:])      # same ops, same workspaces: stream order only
    for (name, *_), r, a, ref in zip(cases, first[0] + second[0], first[1] + second[1], refs):
        assert_same(record(r, a), ref, name)


def test_side_stream(ops):
    cases, refs = prepared(ops, torch.float32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rs, aus = run_batch(ops, cases[2:9])
    s.synchronize()
    for (name, *_), r, a, ref in zip(cases[2:9], rs, aus, refs[2:9]):
        assert_same(record(r, a), ref, name)


def test_argument_errors(ops):
    rank, auc = ops
    cases, _ = prepared(ops, torch.float32)
    lgs, labs = [c[1] for c in cases[:3]], [c[2] for c in cases[:3]]
    with pytest.raises(TypeError):
        rank.batch([lgs[0], lgs[1].bfloat16()])
    with pytest.raises(ValueError):
        rank.batch([])
    with pytest.raises(ValueError):
        rank.batch(lgs, labels_list=labs[:2])
    with pytest.raises(ValueError):
        rank.batch(lgs, labels_list=[labs[0], labs[1][:-1], labs[2]])
    with pytest.raises(ValueError):
        rank.batch([lgs[0], lgs[1].cpu()])
    with pytest.raises(ValueError):
        rank.batch(lgs, k=[1, 16, 1])          # k > n for the 3 x 5 map
    rs = rank.batch(lgs)
    assert rs.hits is None and rs[0].hits is None
    with pytest.raises(ValueError):
        auc.batch([r.probs for r in rs], labs[:2])
    with pytest.raises(ValueError):
        auc.batch([r.probs for r in rs], labs, max_pos=[1, 16, 1])


def test_one_complex_overflows_max_pos(ops):
    """The middle complex has more positives than its max_pos: its neighbours' figures equal the single
    op's, and it equals the single op after the rerun both make on the first read."""
    from deepinteract_amd.ranking import ContactAucOp
    rank, _ = ops
    auc = ContactAucOp("cuda")               # its own workspace: the rerun has to fit it too
    cases = [(f"30 % positives {i}", randn_logits(300, 290 + i, 30 + i, 2.0).cuda(),
              bernoulli(300 * (290 + i), 0.3, 40 + i).cuda(), None) for i in range(3)]
    rs = rank.batch([c[1] for c in cases], labels_list=[c[2] for c in cases])
    aus = auc.batch([r.probs for r in rs], [c[2] for c in cases], max_pos=[None, 1000, None])
    torch.cuda.synchronize()
    raw = [_lib_auc(a) for a in aus]
    assert [m.overflow for m in raw] == [0, 1, 0]
    assert raw[1].num_pos == int(cases[1][2].sum()) and raw[1].num_pos + raw[1].num_neg == 300 * 291
    for i, (name, lg, lab, _) in enumerate(cases):
        single = auc(rs[i].probs, lab, max_pos=1000 if i == 1 else None)
        assert _bits(aus[i].metrics()) == _bits(single.metrics()), name
        assert aus[i].overflow == 0 and aus[i].max_pos == single.max_pos
    assert aus[1].max_pos == raw[1].num_pos > 1000
    against_ref(aus[1], rs[1].probs, cases[1][2], "rerun after overflow inside a batch")


def _lib_auc(a):
    from deepinteract_amd import _lib
    return _lib.DiAucMetrics.from_buffer_copy(a._metrics_dev.cpu().numpy().tobytes())


# ---- end to end
@pytest.fixture(scope="module")
def test_batch_run(ops):
    from deepinteract_amd.graph import GraphBatch
    from deepinteract_amd.modules import LitGINI
    from deepinteract_amd.weights import seeded_state_dict
    zs = [load_case("c1"), load_case("c2")]
    model = LitGINI(dtype="f32", precise_head=True).cuda().eval().load_reference_state_dict(seeded_state_dict(0))
    graphs = [_residue_graph(z, tag) for z in zs for tag in ("g1", "g2")]
    examples = []
    for s, z in enumerate(zs):
        l1, l2 = int(z["logits"].shape[2]), int(z["logits"].shape[3])
        i, j = torch.meshgrid(torch.arange(l1), torch.arange(l2), indexing="ij")
        examples.append(torch.stack((i.flatten(), j.flatten(), bernoulli(l1 * l2, 0.05, 50 + s).long()), dim=1))
    seen = []
    forward = model._forward_batch

    def spy(gb, pairs):              # the logits test_batch judged
        out = forward(gb, pairs)
        seen.append([lg.clone() for lg in out[0]])
        return out

    model._forward_batch = spy
    paths = ["/data/test/4heq_l_u.dill", "/data/test/1abc_r_b.dill"]
    with torch.no_grad():
        gb = GraphBatch.from_graphs(graphs, device=model.engine.device, node_count_limit=model.cfg.node_count_limit)
        outs = model.test_batch(gb, [(0, 1), (2, 3)], examples, paths)
        outs_keep1 = model.test_batch(gb, [(0, 1), (2, 3)], examples, paths, keep_maps=1)
    torch.cuda.synchronize()
    return model, zs, examples, seen, outs, outs_keep1


def test_litgini_test_batch_equals_single_ops(ops, test_batch_run):
    from deepinteract_amd.ranking import confusion_metrics, topk_metrics
    rank, auc = ops
    model, zs, examples, seen, outs, outs_keep1 = test_batch_run
    assert len(outs) == 2 and len(seen) == 2
    keys = {"loss", "top_10_prec", "top_l_by_10_prec", "top_l_by_5_prec", "top_l_recall", "top_l_by_2_recall",
            "top_l_by_5_recall", "test_preds", "test_preds_rounded", "test_labels", "target", "confusion",
            "test_auroc", "test_auprc", "test_acc", "test_prec", "test_recall", "test_f1"}
    for c, (out, z, ex, lg) in enumerate(zip(outs, zs, examples, seen[0])):
        assert set(out) == keys
        l1, l2 = int(lg.shape[2]), int(lg.shape[3])
        lab = ex[:, 2].to(torch.uint8).cuda()
        r = rank(lg.contiguous(), k=min(l1, l2), labels=lab, threshold=model.pos_prob_threshold)
        a = auc(r.probs, lab)
        want = {"loss": r.ce_sum / (l1 * l2), "test_auroc": a.auroc, "test_auprc": a.auprc}
        want.update(topk_metrics(r.hits.cpu(), r.num_pos, min(l1, l2)))
        confusion = {f: getattr(r, f) for f in ("tp", "fp", "fn", "tn")}
        want.update(confusion_metrics(**confusion))
        assert out["confusion"] == confusion
        assert _bits({k: out[k] for k in want}) == _bits(want), c
        assert out["target"] == ("4heq", "1abc")[c]
        assert np.array_equal(out["test_preds"], r.probs.cpu().numpy())
        assert np.array_equal(out["test_labels"], lab.view(l1, l2).float().cpu().numpy())
        assert np.array_equal(out["test_preds_rounded"], (out["test_preds"] >= 0.5).astype(np.float32))
        assert float(np.abs(out["test_preds"] - z["probs"]).max()) <= 1e-4
    # keep_maps = 1: the second dict carries no maps, and the same figures
    assert set(outs_keep1[1]) == keys and outs_keep1[0]["test_preds"] is not None
    assert all(outs_keep1[1][k] is None for k in ("test_preds", "test_preds_rounded", "test_labels"))
    assert outs_keep1[1]["confusion"] == _figures_of(seen[1][1], examples[1], rank, model)


def _figures_of(lg, ex, rank, model):
    r = rank(lg.contiguous(), labels=ex[:, 2].to(torch.uint8).cuda(), threshold=model.pos_prob_threshold)
    return {f: getattr(r, f) for f in ("tp", "fp", "fn", "tn")}


def test_epoch_end_of_test_batch(test_batch_run):
    model, _, _, _, outs, _ = test_batch_run
    got = model.test_epoch_end(outs)
    for name in ("test_acc", "test_prec", "test_recall", "test_f1", "test_auroc", "test_auprc"):
        want = float(torch.median(torch.tensor([o[name] for o in outs], dtype=torch.float64)))
        assert got["med_" + name] == want or (math.isnan(want) and math.isnan(got["med_" + name]))
        assert got["med_" + name] == min(o[name] for o in outs)      # two values: the lower one
